"""Cases, float64 reference and bars of tests/test_gaussian_reg_gpu.py -- CPU only, so that tests/test_gaussian_reg_cpu.py can check
the generator and what the bars are built from without a GPU.

``make_case(P, filtered, selected)``  P rows from a seed (cached, never modified): raw log-scales whose scales lie in about
                         [0.002, 0.3] with log-normal anisotropy (both hinges, ``MAX_RATIO = 10`` and ``MAX_SCALE = 0.05``, have rows on
                         each side), logits in [-8, 8], a filter in [0.001, 0.05], a ``select`` with about 30 % false, six
                         cotangents of mixed sign.  From ``P >= 8`` on, rows 0..6 are planted (``PLANTED``): ties of two raw scales at
                         the minimum and at the maximum, a tie of all three, a logit of +40 and one of -110 (the entropy guard in
                         float32), and, filtered, a row whose ``f`` is 500 times its scales.  Planted rows are always selected.
``check_case(c)``        what keeps float32 and float64 on one branch: every ratio differs from ``MAX_RATIO`` and every scale from
                         ``MAX_SCALE`` by more than 1e-3 relative (on ALL rows, the planted ones too), and every unplanted ``o`` is
                         strictly inside (0, 1) in float32.
``run_torch(c, dt)``     ``gaussian_reg_loss_torch`` in ``dt`` on the host with autograd for ``L = sum_k cot_k terms_k``: (terms (6,),
                         dL/d_opacity (P,1), dL/d_scaling (P,3), count) as float64.  ``reference`` is that in float64 (cached),
                         ``float32_path`` in float32.
``closed_form(c)``       the same from the closed forms written out by hand, in float64, with the three wrong variants of
                         tests/test_gaussian_reg_cpu.py as switches.
``bars(...)``            the project's rule (appearance_cases.bars, depth_prior_cases.bars): 4 x what the float32 statement loses
                         against the float64 statement on the same input, plus 16 float32 epsilons times a scale.  The scale is
                         ``1 + |ref|`` for a term; for a per-row gradient it is ``sum_k |cot_k| |d term_k / d leaf|`` from the closed
                         form, of order 1 / n (a floor of 16 epsilons against 1 would hide any error).  Nothing in a bar comes from
                         the kernel.  Where the scale is 0 (an unselected row) the bar is 0: exact zeros.
"""
import functools
import math

import torch

from bags_raster.gaussian_reg import REG_TERMS, ROWS_PER_GROUP, gaussian_reg_loss_torch

MAX_RATIO, MAX_SCALE = 10.0, 0.05
FACTOR, FLOOR_EPS = 4.0, 16.0
EPS32 = float(torch.finfo(torch.float32).eps)
F32, F64 = torch.float32, torch.float64
SEED = 11
# one row; around a wave; around a workgroup of the backward; around the rows of one workgroup of the sums kernel; several records
SIZES = (1, 63, 64, 65, 255, 256, 257, ROWS_PER_GROUP - 1, ROWS_PER_GROUP, ROWS_PER_GROUP + 1, 3 * ROWS_PER_GROUP + 17)
COMBOS = tuple((f, s) for f in (False, True) for s in (False, True))
PLANTED = {"tie_min": 0, "tie_max": 1, "tie_all": 2, "logit_high": 3, "logit_low": 4, "big_filter": 5, "tie_all_small": 6}
NEAR = 1e-3


def _activated(c, dtype=F64):
    """(o (P,), s (P,3), e (P,3), f2 (P,1), sigmoid (P,), c (P,)) in ``dtype`` from the case's float32 values."""
    x, r = c["opacity"].to(dtype)[:, 0], c["scaling"].to(dtype)
    sig, e = torch.sigmoid(x), torch.exp(r)
    f2 = torch.square(c["filter"].to(dtype)) if c["filtered"] else torch.zeros(r.shape[0], 1, dtype=dtype)
    s = torch.sqrt(e * e + f2) if c["filtered"] else e
    coef = (e / s).prod(1)
    return sig * coef, s, e, f2, sig, coef


def _first(r, largest):
    """The first maximum / minimum of each row of ``r`` (P,3) by strict comparisons."""
    r0, r1, r2 = r.unbind(1)
    better = (lambda a, b: a > b) if largest else (lambda a, b: a < b)                   # noqa: E731
    k = better(r1, r0).long()
    return torch.where(better(r2, torch.where(k == 1, r1, r0)), torch.full_like(k, 2), k)


def check_case(c):
    """What keeps float32 and float64 on the same branch, and the case non-trivial; returns the figures."""
    P = c["P"]
    o64, s, _, _, _, _ = _activated(c)
    kmin, kmax = _first(c["scaling"], False), _first(c["scaling"], True)
    ratio = s.gather(1, kmax[:, None])[:, 0] / s.gather(1, kmin[:, None])[:, 0]
    gap_ratio = float((ratio / MAX_RATIO - 1).abs().min()) if P else 1.0
    gap_scale = float((s / MAX_SCALE - 1).abs().min()) if P else 1.0
    assert gap_ratio > NEAR and gap_scale > NEAR, (gap_ratio, gap_scale)
    o32 = _activated(c, F32)[0]
    plain = ~c["planted"]
    assert bool(((o32 > 0) & (o32 < 1))[plain].all())
    fig = dict(gap_ratio=gap_ratio, gap_scale=gap_scale, n=int(c["sel"].sum()))
    if P >= 63:                                              # both hinges have selected rows on each side; some rows are not selected
        sel = c["sel"]
        assert bool((ratio > MAX_RATIO)[sel].any()) and bool((ratio < MAX_RATIO)[sel].any())
        assert bool((s > MAX_SCALE)[sel].any()) and bool((s < MAX_SCALE)[sel].any())
        assert (not c["selected"]) or 0.5 * P < fig["n"] < 0.9 * P
    return fig


@functools.lru_cache(maxsize=None)
def make_case(P, filtered, selected, seed=SEED):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * P + 2 * int(filtered) + int(selected))
    size = math.log(0.009) + (math.log(0.067) - math.log(0.009)) * torch.rand(P, 1, generator=g)
    scaling = size + torch.randn(P, 3, generator=g).clamp(-1.5, 1.5)                     # scales in [0.002, 0.3]
    opacity = 16.0 * torch.rand(P, 1, generator=g) - 8.0
    filt = torch.exp(math.log(0.001) + (math.log(0.05) - math.log(0.001)) * torch.rand(P, 1, generator=g))
    sel = torch.rand(P, generator=g) >= 0.3 if selected else torch.ones(P, dtype=torch.bool)
    cot = (0.5 + torch.rand(6, generator=g)) * torch.tensor([1.0, -1.0, 1.0, -1.0, 1.0, -1.0])
    planted = torch.zeros(P, dtype=torch.bool)
    if P >= 8:
        a, b = math.log(0.01), math.log(0.03)
        k = PLANTED
        scaling[k["tie_min"]] = torch.tensor([a, a, b])
        scaling[k["tie_max"]] = torch.tensor([a, b, b])
        scaling[k["tie_all"]] = math.log(0.08)
        scaling[k["tie_all_small"]] = a
        opacity[k["logit_high"]], opacity[k["logit_low"]] = 40.0, -110.0
        scaling[k["big_filter"]] = torch.tensor([a, b, a + 0.3])
        filt[[k["tie_min"], k["tie_max"], k["tie_all"], k["tie_all_small"]]] = 0.02
        if filtered:
            filt[k["big_filter"]] = 5.0
        planted[list(k.values())] = True
        sel = sel | planted
        if selected:
            sel[7] = False
    elif selected:
        sel[0] = True
        if P >= 2:
            sel[1] = False
    c = dict(P=P, filtered=filtered, selected=selected, opacity=opacity, scaling=scaling, filter=filt, sel=sel, cot=cot, planted=planted)
    # move what sits within 2e-3 of a hinge (float32 and float64 must agree on both): a scale first, then the ratio
    for _ in range(8):
        _, s, _, _, _, _ = _activated(c)
        near = (s / MAX_SCALE - 1).abs() <= 2 * NEAR                                    # (no planted scale is)
        kmin, kmax = _first(scaling, False), _first(scaling, True)
        ratio = s.gather(1, kmax[:, None])[:, 0] / s.gather(1, kmin[:, None])[:, 0]
        near_ratio = (ratio / MAX_RATIO - 1).abs() <= 2 * NEAR
        if not (near.any() or near_ratio.any()):
            break
        scaling += 0.01 * near.float()
        filt[near.any(1)] *= 0.97                            # (a scale that is mostly filter does not move with its raw value)
        scaling[near_ratio, kmax[near_ratio]] += 0.01
    c["figures"] = check_case(c)
    return c


def run_torch(c, dtype):
    """(terms (6,), dL/d_opacity (P,1), dL/d_scaling (P,3), count) of gaussian_reg_loss_torch in ``dtype`` on the host for
    L = sum_k cot_k terms_k, as float64."""
    x = c["opacity"].detach().clone().to(dtype).requires_grad_(True)                     # the cached case stays as it is
    r = c["scaling"].detach().clone().to(dtype).requires_grad_(True)
    terms, count = gaussian_reg_loss_torch(x, r, c["filter"].to(dtype) if c["filtered"] else None, c["sel"] if c["selected"] else None,
                                           REG_TERMS, MAX_RATIO, MAX_SCALE)
    assert terms.dtype == dtype and tuple(terms.shape) == (6,) and count.dtype == dtype and not count.requires_grad
    (terms.double() * c["cot"].double()).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad                   # noqa: E731
    return terms.detach().double(), zero(x).double(), zero(r).double(), count.detach().double()


@functools.lru_cache(maxsize=None)
def reference(P, filtered, selected):
    return run_torch(make_case(P, filtered, selected), F64)


@functools.lru_cache(maxsize=None)
def float32_path(P, filtered, selected):
    return run_torch(make_case(P, filtered, selected), F32)


def _term_gradients(c, drop_through_c=False, n_not_3n=False, flat_argmax=False):
    """The closed forms in float64: (sums (6,) of the selected rows' terms before the division, divisors (6,), d term_k / d x (6,P),
    d term_k / d r (6,P,3)), the division included in the derivatives.  The switches are the three wrong answers."""
    P = c["P"]
    o, s, e, f2, sig, coef = _activated(c)
    sel = (c["sel"] if c["selected"] else torch.ones(P, dtype=torch.bool))
    w = sel.double()
    n = float(w.sum())
    inv_n = 1.0 / n if n > 0 else 0.0
    third = inv_n if n_not_3n else inv_n / 3.0
    kmin, kmax = _first(c["scaling"], False), _first(c["scaling"], True)
    at_min, at_max = torch.nn.functional.one_hot(kmin, 3).double(), torch.nn.functional.one_hot(kmax, 3).double()
    s_min, s_max = (s * at_min).sum(1), (s * at_max).sum(1)
    ratio = s_max / s_min
    over, big = (ratio - MAX_RATIO > 0).double(), (s - MAX_SCALE > 0).double()
    inside = (o > 0) & (o < 1)
    o_in = torch.where(inside, o, torch.full_like(o, 0.5))
    ent = torch.where(inside, -(o_in * torch.log(o_in) + (1 - o_in) * torch.log(1 - o_in)), torch.zeros_like(o))
    flat_pick = at_max if flat_argmax else at_min
    sums = torch.stack([(w * o).sum(), (w * s.sum(1)).sum(), (w * (s * flat_pick).sum(1)).sum(), (w * over * (ratio - MAX_RATIO)).sum(),
                        (w[:, None] * big * (s - MAX_SCALE)).sum(), (w * ent).sum()])
    div = torch.tensor([inv_n, third, inv_n, inv_n, third, inv_n], dtype=F64)
    # the activations' derivatives: do/dx, do/dr_a (through c), ds_a/dr_a
    do_dx = coef * sig * (1 - sig)
    do_dr = torch.zeros(P, 3, dtype=F64) if drop_through_c else (sig * coef)[:, None] * f2 / (s * s)
    ds_dr = e * e / s
    # d term_k / d o (P,) and d term_k / d s_a (P,3)
    d_o = torch.zeros(6, P, dtype=F64)
    d_s = torch.zeros(6, P, 3, dtype=F64)
    d_o[0] = inv_n
    d_o[5] = torch.where(inside, torch.log(1 - o_in) - torch.log(o_in), torch.zeros_like(o)) * inv_n
    d_s[1] = third
    d_s[2] = flat_pick * inv_n
    d_s[3] = over[:, None] * (at_max / s_min[:, None] - at_min * (s_max / (s_min * s_min))[:, None]) * inv_n
    d_s[4] = big * third
    g_x = d_o * do_dx * w
    g_r = (d_s * ds_dr + d_o[:, :, None] * do_dr) * w[:, None]
    return sums, div, g_x, g_r


def closed_form(c, **wrong):
    """(terms (6,), dL/d_opacity (P,1), dL/d_scaling (P,3)) from the closed forms, in float64, the cotangents included."""
    sums, div, g_x, g_r = _term_gradients(c, **wrong)
    cot = c["cot"].double()
    return sums * div, (cot[:, None] * g_x).sum(0)[:, None], (cot[:, None, None] * g_r).sum(0)


def scales(c):
    """sum_k |cot_k| |d term_k / d leaf| of the closed forms in float64: (dL/d_opacity (P,1), dL/d_scaling (P,3))."""
    _, _, g_x, g_r = _term_gradients(c)
    cot = c["cot"].double().abs()
    return (cot[:, None] * g_x.abs()).sum(0)[:, None], (cot[:, None, None] * g_r.abs()).sum(0)


def bars_of(c, r64, r32):
    """(bar of the terms, of dL/d_opacity, of dL/d_scaling) from the two runs of the statement and the case's scales."""
    s_x, s_r = scales(c)
    lost = [FACTOR * (b - a).abs() for a, b in zip(r64[:3], r32[:3])]
    return lost[0] + FLOOR_EPS * EPS32 * (1 + r64[0].abs()), lost[1] + FLOOR_EPS * EPS32 * s_x, lost[2] + FLOOR_EPS * EPS32 * s_r


@functools.lru_cache(maxsize=None)
def bars(P, filtered, selected):
    return bars_of(make_case(P, filtered, selected), reference(P, filtered, selected), float32_path(P, filtered, selected))


def margins_of(bar, ref, got):
    """Largest error over bar of each of (terms, dL/d_opacity, dL/d_scaling) against ``ref``; where a bar is 0 the value must be the
    reference's exactly (an unselected row: zeros), which counts as margin 0 -- anything else, and any NaN, as infinity."""
    m = []
    for b, r, g in zip(bar, ref[:3], got[:3]):
        err = (g.detach().double().cpu() - r).abs()
        ratio = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), ratio)
        m.append(float(ratio.max()) if ratio.numel() else 0.0)
    return tuple(m)


def margins(P, filtered, selected, got):
    return margins_of(bars(P, filtered, selected), reference(P, filtered, selected), got)
