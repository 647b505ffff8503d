"""Cases, float64 reference and bars of tests/test_depth_prior_gpu.py -- CPU only, so that tests/test_depth_prior_cpu.py can check
the generators and what the bars are built from without a GPU.

``make_case(H, W, V, mode, space)``  V views of ``H x W``: ``z`` in [2,5], ``A`` in [0.55,1] with a tenth of the pixels far below
                         ``min_weight = 0.5``, ``D = A z``; a prior that follows ``z`` (``1/z`` for ``space="inverse"``) with 10 %
                         noise, a twentieth of it zeros and a few NaN; a mask with a tenth zeros and three tenths fractional; an
                         unordered list of V distinct rows of an ``N = 23`` table with ``|a - 1|, |b| <= 0.2``; per-view cotangents
                         of mixed sign; all from a seed (cached, never modified).  The generator asserts what keeps float32 and
                         float64 on the same branch (``check_case``).
``degenerate_case(mode, space)``     the 16-view case of 17 x 67 with four views replaced: no valid pixel, one valid pixel, an exactly
                         constant prior, an all-zero mask.
``run_torch(case, dt)``  ``depth_prior_loss_torch`` in ``dt`` on the host with autograd: (loss, dL/dD, dL/dA, dL/dtable rows) as
                         float64 tensors.  ``reference`` is that in float64 (cached), ``float32_path`` in float32.
``closed_form(case)``    the same four from the closed forms of the issue, in float64, with the three wrong variants of
                         tests/test_depth_prior_cpu.py as switches.
``bars(...)``            the project's rule (appearance_cases.bars): 4 x what the float32 statement loses against the float64
                         statement on the same input, plus 16 float32 epsilons times a scale.  The scale is ``1 + |ref|`` for the
                         loss; for a per-pixel gradient the sum of the absolute values of the terms of its closed form, with the
                         differences ``p - pbar`` and ``x - xbar`` counted as two terms each (``x`` carries a float32 rounding
                         proportional to ``|x|``, not to ``|x - xbar|``) -- the gradients are of order 1 / (H W), and a floor of 16
                         epsilons against 1 would hide any error; for a table gradient ``sum |terms| / n``.  Nothing in a bar comes
                         from the kernel.  Where the scale is 0 (an invalid pixel, a degenerate view) the bar is 0: exact zeros.
"""
import functools

import torch

from bags_raster import _lib as L
from bags_raster.depth_prior import DEGENERATE, depth_prior_loss_torch

N = 23                                                       # rows of the table
MIN_WEIGHT = 0.5
CHAIN_MIN_WEIGHT = 0.87                                      # of the chain through the real operator (tests/test_depth_prior_gpu.py):
                                                             # the scene's weights lie in [0.861, 0.955], three pixels below 0.87
FACTOR, FLOOR_EPS = 4.0, 16.0
EPS32 = float(torch.finfo(torch.float32).eps)
F64 = torch.float64
MODES, SPACES = ("pearson", "l1"), ("depth", "inverse")

QUADS_PER_TILE = L.DEPTH_PRIOR_BLOCK                         # a thread takes a quad of 4 pixels, a workgroup a tile of 256 quads


def tiles(H, W):
    return -(-(H * ((W + 3) // 4)) // QUADS_PER_TILE)


def slots(H, W):
    """Workgroups per view of the sums kernel (include/bags_raster.h: BAGS_DEPTH_PRIOR_*)."""
    t = tiles(H, W)
    return min(t, max(L.DEPTH_PRIOR_MIN_SLOTS, -(-t // L.DEPTH_PRIOR_TILES_PER_SLOT)))


def _strided_shape():
    """From the kernel's constants: whole quads (the vector path is eligible), more tiles than a view has workgroups, so some
    workgroups walk two tiles, and a last tile that is not full."""
    W = 520
    H = (L.DEPTH_PRIOR_MIN_SLOTS * QUADS_PER_TILE) // (W // 4) + 1
    assert W % 4 == 0 and tiles(H, W) > slots(H, W) >= 2 and (H * (W // 4)) % QUADS_PER_TILE != 0 and H <= 160 and W <= 520
    return H, W


STRIDED = _strided_shape()                                   # (127, 520) with 256 / 64 / 4
SHAPES = ((1, 1), (3, 5), (16, 64), (17, 67), (37, 259), STRIDED)
VIEWS = (1, 2, 16, 17)
SEED = 3


def _pieces(c):
    """The float64 pieces of the closed forms for the case's maps as they are (x formed in float64): a dict of (V,H,W) tensors
    and (V,) sums."""
    D, A, p, m = c["D"][:, 0].double(), c["A"][:, 0].double(), c["prior"].double(), c["mask"].double()
    valid = (m > 0) & (A >= MIN_WEIGHT) & (D > 0) & (p > 0)
    one = torch.ones((), dtype=F64)
    Dv, Av, pv = torch.where(valid, D, one), torch.where(valid, A, one), torch.where(valid, p, one)
    w = torch.where(valid, m, torch.zeros((), dtype=F64))
    if c["space"] == "inverse":
        x, dxdD, dxdA = Av / Dv, -Av / (Dv * Dv), 1.0 / Dv
    else:
        x, dxdD, dxdA = Dv / Av, 1.0 / Av, -Dv / (Av * Av)
    n = w.sum((1, 2))
    s = lambda t: t.sum((1, 2)) / n.clamp_min(1e-300)                                   # noqa: E731
    ab = c["table"][c["rows"]].double()
    r = x - (ab[:, 0, None, None] * pv + ab[:, 1, None, None])
    xbar, pbar, ex2, ep2 = s(w * x), s(w * pv), s(w * x * x), s(w * pv * pv)
    Vx, Vp, Cxp = ex2 - xbar ** 2, ep2 - pbar ** 2, s(w * x * pv) - xbar * pbar
    return dict(valid=valid, x=x, p=pv, w=w, n=n, r=r, dxdD=dxdD, dxdA=dxdA, xbar=xbar, pbar=pbar, ex2=ex2, ep2=ep2, Vx=Vx, Vp=Vp, Cxp=Cxp, ab=ab)


def check_case(c):
    """What keeps float32 and float64 on the same branch, and the case non-trivial; returns the figures."""
    q = _pieces(c)
    H, W, V = c["H"], c["W"], c["V"]
    A = c["A"].double()
    gap = float((A - MIN_WEIGHT).abs().min())
    assert gap >= 1e-3, gap                                                               # no A within 1e-3 of min_weight
    live = [v for v in range(V) if v not in c["degenerate"]]
    share = float(q["valid"][live].double().mean()) if live else 1.0
    assert share >= 0.5, share                                                            # at least half of the pixels valid
    rmin = float(q["r"].abs()[q["valid"]].min()) if q["valid"].any() else 1.0
    if c["mode"] == "l1":
        assert rmin >= 1e-4, rmin                                                         # no valid |r| below 1e-4
    cond = 1.0
    if c["mode"] == "pearson":
        for v in live:
            assert q["n"][v] > 0
            cond = min(cond, float(q["Vx"][v] / q["ex2"][v]), float(q["Vp"][v] / q["ep2"][v]))
        assert cond >= 1e-3, cond                                                         # Vx, Vp above 1e-3 of their mean squares
    return dict(gap=gap, valid=share, rmin=rmin, cond=cond)


@functools.lru_cache(maxsize=None)
def make_case(H, W, V, mode, space, seed=SEED):
    assert mode in MODES and space in SPACES
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * H + 31 * W + V + (500009 if space == "inverse" else 0))
    px = H * W
    z = 2.0 + 3.0 * torch.rand(V, px, generator=g)
    A = 0.55 + 0.45 * torch.rand(V, px, generator=g)
    prior = (1.0 / z if space == "inverse" else z) * (1.0 + 0.1 * torch.randn(V, px, generator=g).clamp(-3, 3))
    mask = torch.ones(V, px)
    table = torch.stack([1.0 + 0.2 * (torch.rand(N, generator=g) * 2 - 1), 0.2 * (torch.rand(N, generator=g) * 2 - 1)], 1)
    if space == "inverse":
        table[:, 1] *= 0.2                                   # an inverse depth is in [0.2, 0.5]: |b| <= 0.04
    rows = torch.randperm(N, generator=g)[:V].tolist()
    if rows == sorted(rows):                                 # unordered for every V > 1
        rows.reverse()
    n_low, n_zero, n_nan, n_off, n_frac = px // 10, px // 20, (max(1, px // 200) if px >= 8 else 0), px // 10, (3 * px) // 10
    for v in range(V):                                       # distinct places per kind; the kinds may overlap
        A[v, torch.randperm(px, generator=g)[:n_low]] = 0.3 * torch.rand(n_low, generator=g)
        prior[v, torch.randperm(px, generator=g)[:n_zero]] = 0.0
        prior[v, torch.randperm(px, generator=g)[:n_nan]] = float("nan")
        at = torch.randperm(px, generator=g)
        mask[v, at[:n_off]] = 0.0
        mask[v, at[n_off:n_off + n_frac]] = 0.1 + 0.9 * torch.rand(n_frac, generator=g)
    if px == 1:
        mask[:] = 0.75                                       # n != H W also for a single pixel
    D = A * z
    # l1: move a prior whose residual would be too close to the kink of |r| (float32 and float64 must agree on sign(r))
    ab = table[rows].double()
    x = (A.double() / D.double()) if space == "inverse" else (D.double() / A.double())
    r = x - (ab[:, 0, None] * prior.double() + ab[:, 1, None])
    near = r.abs() < (2e-3 if space == "depth" else 4e-4)
    prior = torch.where(near, prior * 1.02 + 0.004, prior)
    cot = (0.5 + torch.rand(V, generator=g)) * torch.where(torch.arange(V) % 2 == 0, 1.0, -1.0)
    degenerate = tuple(range(V)) if (mode == "pearson" and px == 1) else ()              # one pixel has no variance
    c = dict(H=H, W=W, V=V, mode=mode, space=space, D=D.view(V, 1, H, W), A=A.view(V, 1, H, W), prior=prior.view(V, H, W).contiguous(),
             mask=mask.view(V, H, W), table=table, rows=rows, cot=cot, degenerate=degenerate)
    c["figures"] = check_case(c)
    return c


DEGENERATE_VIEWS = {"none_valid": 2, "one_valid": 5, "constant_prior": 9, "mask_zero": 12}


@functools.lru_cache(maxsize=None)
def degenerate_case(mode, space):
    """The 16-view case of 17 x 67 with the four views of DEGENERATE_VIEWS replaced; the other twelve are that case's."""
    base = make_case(17, 67, 16, mode, space)
    c = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in base.items()}
    k = DEGENERATE_VIEWS
    c["prior"][k["none_valid"]] = torch.where(torch.arange(17 * 67).view(17, 67) % 2 == 0, 0.0, float("nan"))
    one = torch.zeros(17, 67)
    ok = ((c["A"][k["one_valid"], 0] >= MIN_WEIGHT) & (c["prior"][k["one_valid"]] > 0)).nonzero()[7]
    one[ok[0], ok[1]] = 0.625
    c["mask"][k["one_valid"]] = one
    # not a short binary fraction, and above every a x + b of the view: no l1 residual is near the kink of |r|
    c["prior"][k["constant_prior"]] = 0.8137 if space == "inverse" else 7.137
    c["mask"][k["mask_zero"]] = 0.0
    # pearson: all four have no correlation; l1: the two without a valid pixel have no loss, the other two are ordinary views
    c["degenerate"] = tuple(sorted(k.values())) if mode == "pearson" else (k["none_valid"], k["mask_zero"])
    c["figures"] = check_case(c)
    return c


def run_torch(c, dtype, views=None):
    """(loss (V,), dL/dD (V,1,H,W), dL/dA (V,1,H,W), dL/dtable rows (V,2) or None) of depth_prior_loss_torch in ``dtype`` on the
    host for L = sum cot_v loss_v, as float64, and the count (V,)."""
    idx = list(range(c["V"])) if views is None else list(views)
    D = [c["D"][i].detach().clone().to(dtype).requires_grad_(True) for i in idx]        # the cached case stays as it is
    A = [c["A"][i].detach().clone().to(dtype).requires_grad_(True) for i in idx]
    kw = {}
    if c["mode"] == "l1":
        table = c["table"].detach().clone().to(dtype).requires_grad_(True)
        kw = dict(table=table, rows=[c["rows"][i] for i in idx])
    loss, count = depth_prior_loss_torch(D, A, [c["prior"][i].to(dtype) for i in idx], [c["mask"][i].to(dtype) for i in idx],
                                         mode=c["mode"], space=c["space"], min_weight=MIN_WEIGHT, **kw)
    assert loss.dtype == dtype and count.dtype == dtype and not count.requires_grad
    (loss.double() * c["cot"][idx].double()).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad                   # noqa: E731
    g_rows = None
    if c["mode"] == "l1":
        g = table.grad.detach().double()
        other = [r for r in range(N) if r not in kw["rows"]]
        assert not other or bool((g[other] == 0).all())
        g_rows = g[kw["rows"]]
    return (loss.detach().double(), torch.stack([zero(t) for t in D]).double(), torch.stack([zero(t) for t in A]).double(), g_rows,
            count.detach().double())


@functools.lru_cache(maxsize=None)
def reference(H, W, V, mode, space):
    return run_torch(make_case(H, W, V, mode, space), F64)


@functools.lru_cache(maxsize=None)
def float32_path(H, W, V, mode, space):
    return run_torch(make_case(H, W, V, mode, space), torch.float32)


def closed_form(c, drop_rho=False, flip_dA=False, n_is_pixels=False):
    """(loss, dL/dD, dL/dA, dL/dtable rows or None) from the closed forms, in float64, the cotangent included.  The switches
    make the three wrong answers the bars must reject: the ``rho (x - xbar) / Vx`` term dropped, the sign of dx/dA flipped, 1/n of
    the gradient replaced by 1 / (H W)."""
    q = _pieces(c)
    V = c["V"]
    n, w, x, p = q["n"], q["w"], q["x"], q["p"]
    inv_n = torch.where(n > 0, 1.0 / n.clamp_min(1e-300), torch.zeros_like(n))
    inv_g = torch.full_like(n, 1.0 / (c["H"] * c["W"])) if n_is_pixels else inv_n
    e = lambda t: t[:, None, None]                                                       # noqa: E731
    g_rows = None
    if c["mode"] == "l1":
        sg = torch.sign(q["r"])
        loss = (w * q["r"].abs()).sum((1, 2)) * inv_n
        gx = w * sg * e(inv_g)
        g_rows = torch.stack([-(w * sg * p).sum((1, 2)) * inv_g, -(w * sg).sum((1, 2)) * inv_g], 1) * c["cot"].double()[:, None]
    else:
        live = (n > 0) & (q["Vx"] > DEGENERATE * q["ex2"]) & (q["Vp"] > DEGENERATE * q["ep2"])
        k1 = 1.0 / torch.sqrt(torch.where(live, q["Vx"] * q["Vp"], torch.ones_like(n)))
        rho = q["Cxp"] * k1
        loss = torch.where(live, 1.0 - rho, torch.zeros_like(n))
        k2 = torch.zeros_like(n) if drop_rho else rho / torch.where(live, q["Vx"], torch.ones_like(n))
        gx = -(w * e(inv_g)) * ((p - e(q["pbar"])) * e(k1) - e(k2) * (x - e(q["xbar"])))
        gx = gx * e(live.double())
    gx = gx * e(c["cot"].double())
    assert set(v for v in range(V) if c["mode"] == "pearson" and not live[v]) <= set(c["degenerate"])
    return loss, (gx * q["dxdD"])[:, None], (gx * q["dxdA"] * (-1.0 if flip_dA else 1.0))[:, None], g_rows


def scales(c):
    """sum |terms| of the closed forms in float64: (loss (V,), dL/dD (V,1,H,W), dL/dA (V,1,H,W), dL/dtable rows (V,2) or None)."""
    q = _pieces(c)
    n, w, x, p = q["n"], q["w"], q["x"], q["p"]
    inv_n = torch.where(n > 0, 1.0 / n.clamp_min(1e-300), torch.zeros_like(n))
    e = lambda t: t[:, None, None]                                                       # noqa: E731
    cot = c["cot"].double().abs()
    g_rows = None
    if c["mode"] == "l1":
        t = w * e(inv_n)
        g_rows = torch.stack([(w * p).sum((1, 2)) * inv_n, w.sum((1, 2)) * inv_n], 1) * cot[:, None]
    else:
        live = (n > 0) & (q["Vx"] > DEGENERATE * q["ex2"]) & (q["Vp"] > DEGENERATE * q["ep2"])
        k1 = 1.0 / torch.sqrt(torch.where(live, q["Vx"] * q["Vp"], torch.ones_like(n)))
        k2 = (q["Cxp"] * k1).abs() / torch.where(live, q["Vx"], torch.ones_like(n))
        t = (w * e(inv_n)) * ((p + e(q["pbar"].abs())) * e(k1) + e(k2) * (x + e(q["xbar"].abs()))) * e(live.double())
    t = t * e(cot)
    return None, (t * q["dxdD"].abs())[:, None], (t * q["dxdA"].abs())[:, None], g_rows


def bars_of(c, r64, r32):
    """(bar of loss, of dL/dD, of dL/dA, of dL/dtable rows or None) from the two runs of the statement and the case's scales."""
    _, sD, sA, sT = scales(c)
    lost = [None if a is None else FACTOR * (b - a).abs() for a, b in zip(r64[:4], r32[:4])]
    return (lost[0] + FLOOR_EPS * EPS32 * (1 + r64[0].abs()), lost[1] + FLOOR_EPS * EPS32 * sD, lost[2] + FLOOR_EPS * EPS32 * sA,
            None if sT is None else lost[3] + FLOOR_EPS * EPS32 * sT)


@functools.lru_cache(maxsize=None)
def bars(H, W, V, mode, space):
    return bars_of(make_case(H, W, V, mode, space), reference(H, W, V, mode, space), float32_path(H, W, V, mode, space))


def margins_of(bar, ref, got):
    """Largest error over bar of each of (loss, dL/dD, dL/dA, dL/dtable rows) against ``ref``; where a bar is 0 the value must be
    the reference's exactly (an invalid pixel, a degenerate view: zeros), which counts as margin 0 -- anything else as infinity."""
    m = []
    for b, r, g in zip(bar, ref[:4], got):
        if b is None:
            continue
        err = (g.detach().double().cpu() - r).abs()
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
        m.append(float(ratio.max()))
    return tuple(m)


def margins(H, W, V, mode, space, got):
    return margins_of(bars(H, W, V, mode, space), reference(H, W, V, mode, space), got)
