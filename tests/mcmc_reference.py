"""Reference side of the MCMC tests: the four functions of the 3DGS-MCMC strategy in plain PyTorch, on any device and in fp32 or
fp64 -- ``compute_relocation`` (bags_raster.compute_relocation_torch: the published kernel's double loop, and here its hockey-stick
form), ``relocate_gs`` / ``add_new_gs`` with their optimizer surgery (``_update_params``, ``densification_postfix``,
``replace_tensors_to_optimizer``) and the per-iteration noise step of train.py.  Never the code under test.

The optimizer holds the six groups of ``adam_reference.NAMES`` in that order, one parameter each; ``stats`` is a dict of
``xyz_gradient_accum (P,1)``, ``denom (P,1)``, ``max_radii2D (P)``.  Sampling is no part of the restatement: ``sampled`` is given.

The yardstick (``assert_yardstick``): against the fp64 statement from the same fp32 inputs, the kernel's error may be at most twice
the error of the fp32 statement.  No tolerance is fixed in advance.
"""
import math

import torch

import adam_reference as R
from bags_raster import compute_relocation_torch, relocation_binoms
from densify_reference import build_rotation, params

N_MAX = 51
EPS_CLAMP = float(torch.finfo(torch.float32).eps)


def compute_relocation(opacity_old, scale_old, N, binoms=None, n_max=N_MAX):
    return compute_relocation_torch(opacity_old, scale_old, N, relocation_binoms(n_max) if binoms is None else binoms, n_max)


def compute_relocation_hockey(opacity_old, scale_old, N, n_max=N_MAX):
    """The same function with the double sum folded by the hockey-stick identity sum_{i=k+1..n} C(i-1, k) = C(n, k+1):
    denom = sum_{k=0..n-1} C(n, k+1) (-1)^k o_new^(k+1) / sqrt(k+1), binomials exact."""
    o = opacity_old.reshape(-1)
    n = N.reshape(-1).to(torch.int64).clamp(1, n_max - 1)
    o_new = 1 - torch.pow(1 - o, 1 / n.to(o.dtype))
    denom = torch.zeros_like(o)
    for r in range(o.numel()):
        nr = int(n[r])
        denom[r] = sum(math.comb(nr, k + 1) * (-1.0) ** k / math.sqrt(k + 1) * o_new[r] ** (k + 1) for k in range(nr))
    return o_new.reshape(opacity_old.shape), (o / denom).unsqueeze(-1) * scale_old


def rel_err(x, ref64):
    """max |x - ref| / |ref| over the elements (0 where both are equal); NaN anywhere -> NaN -> every comparison fails."""
    x, ref = x.detach().to("cpu", torch.float64), ref64.detach().to("cpu", torch.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    d = (x - ref).abs()
    return torch.where(d == 0, torch.zeros_like(d), d / ref.abs()).max().item()


def assert_yardstick(label, kernel, ref32, ref64, measure=rel_err):
    ek, e32 = measure(kernel, ref64), measure(ref32, ref64)
    print(f"MCMC_ERR {label}: kernel {ek:.4e} torch_fp32 {e32:.4e} bound {2 * e32:.4e}")
    assert ek <= 2.0 * e32, f"{label}: err(kernel) = {ek:.4e} > 2 * err(torch fp32) = {2 * e32:.4e}"
    return ek, e32


def new_values(p, sampled, min_opacity=0.005, n_max=N_MAX):
    """``_update_params``: (new raw opacity (D,1), new raw scaling (D,3)) of the rows ``sampled``, counts by ``bincount``."""
    P = p["xyz"].shape[0]
    ratio = torch.bincount(sampled, minlength=P)
    o_new, s_new = compute_relocation(torch.sigmoid(p["opacity"].detach()[sampled, 0]), torch.exp(p["scaling"].detach()[sampled]), ratio[sampled] + 1,
                                      n_max=n_max)
    o_new = torch.clamp(o_new.unsqueeze(-1), max=1.0 - EPS_CLAMP, min=min_opacity)
    return torch.log(o_new / (1 - o_new)), torch.log(s_new.reshape(-1, 3))


def _zero_moments(opt, rows):
    """``replace_tensors_to_optimizer(inds=rows)``: both moments of the rows zeroed in every group that has state."""
    for g in opt.param_groups:
        st = opt.state.get(g["params"][0], None)
        if st is not None and "exp_avg" in st:
            st["exp_avg"][rows] = 0
            st["exp_avg_sq"][rows] = 0


@torch.no_grad()
def relocate(opt, dead_mask, sampled, min_opacity=0.005):
    """``relocate_gs`` on ``opt`` in place: dead row j takes row ``sampled[j]`` with the new opacity and scaling, the sources get the
    same two, their moments are zeroed.  Returns {"dead", "sources"}."""
    p = params(opt)
    P = p["xyz"].shape[0]
    dead = dead_mask.nonzero().reshape(-1)
    D = int(dead.numel())
    if D == 0 or D == P:
        return {"dead": D, "sources": 0}
    assert sampled.shape == (D,) and not bool(dead_mask[sampled].any())
    new_op, new_sc = new_values(p, sampled, min_opacity)
    for n in R.NAMES:
        p[n].data[dead] = {"opacity": new_op, "scaling": new_sc}.get(n, p[n].detach()[sampled])
    p["opacity"].data[sampled] = new_op
    p["scaling"].data[sampled] = new_sc
    _zero_moments(opt, sampled)
    return {"dead": D, "sources": int(torch.unique(sampled).numel())}


@torch.no_grad()
def add_new(opt, cap_max, sampled, min_opacity=0.005):
    """``add_new_gs`` on ``opt``: new parameters of P + A rows (``cat_tensors_to_optimizer``), the sources updated as in ``relocate``.
    Returns {"added", "P_new", "stats"}: the statistics are zeros of the new size (``densification_postfix``)."""
    p = params(opt)
    P = p["xyz"].shape[0]
    dev, dt = p["xyz"].device, p["xyz"].dtype
    A = max(0, min(int(cap_max), int(1.05 * P)) - P)
    if A == 0:
        return {"added": 0, "P_new": P, "stats": None}
    assert sampled.shape == (A,)
    new_op, new_sc = new_values(p, sampled, min_opacity)
    ext = [{"opacity": new_op, "scaling": new_sc}.get(n, p[n].detach()[sampled]) for n in R.NAMES]
    p["opacity"].data[sampled] = new_op
    p["scaling"].data[sampled] = new_sc
    R.cat_tensors_to_optimizer(opt, ext)
    _zero_moments(opt, sampled)
    stats = {"xyz_gradient_accum": torch.zeros(P + A, 1, device=dev, dtype=dt), "denom": torch.zeros(P + A, 1, device=dev, dtype=dt),
             "max_radii2D": torch.zeros(P + A, device=dev, dtype=dt)}
    return {"added": A, "P_new": P + A, "stats": stats}


def gate(opacity, k=100.0, x0=0.995):
    """train.py's ``op_sigmoid(1 - get_opacity)``."""
    return 1 / (1 + torch.exp(-k * ((1 - torch.sigmoid(opacity)) - x0)))


def mcmc_noise(xyz, opacity, scaling, rotation, scale, z, k=100.0, x0=0.995, scaling_modifier=1.0):
    """The new xyz of the SGLD step: xyz + Sigma (z g scale), Sigma = L L^T, L = R diag(scaling_modifier exp(scaling))."""
    L = build_rotation(rotation) * (scaling_modifier * torch.exp(scaling)).unsqueeze(1)
    cov = L @ L.transpose(1, 2)
    step = z * gate(opacity, k, x0) * scale
    return xyz + torch.bmm(cov, step.unsqueeze(-1)).squeeze(-1)


# ---------------------------------------------------------------------------------------------------------- test inputs
def relocation_inputs(P, seed, lo=0.005, hi=0.99):
    """fp32 CPU inputs of compute_relocation: opacity uniform in (lo, hi), scales log-uniform, N cycling through 1..50 with the
    out-of-range values 0, 51 and 1000 mixed in (every P >= 53 sees all of them)."""
    g = torch.Generator().manual_seed(seed)
    o = lo + (hi - lo) * torch.rand(P, generator=g)
    s = torch.exp(torch.randn(P, 3, generator=g) - 3.0)
    cycle = torch.tensor(list(range(1, 51)) + [0, 51, 1000], dtype=torch.int32)
    N = cycle[(torch.arange(P) + int(torch.randint(0, 53, (1,), generator=g))) % 53] if P > 1 else torch.tensor([7], dtype=torch.int32)
    return o, s, N


def make_case(P, seed, opt_cls=torch.optim.Adam, device="cpu", sh_degree=3, state=True):
    """An optimizer of ``opt_cls`` over P random Gaussians with real-looking moments (``step`` = 5), or without state; the
    statistics (nonzero, so that a resize shows).  Opacities span (0.005, 0.99)."""
    g = torch.Generator().manual_seed(seed)
    K = (sh_degree + 1) ** 2
    shapes = ((3,), (1, 3), (K - 1, 3), (1,), (3,), (4,))
    states = R.random_state(P, seed, shapes=shapes)
    o = 0.005 + 0.985 * torch.rand(P, 1, generator=g)
    states[3]["param"] = torch.log(o / (1 - o))
    states[4]["param"] = torch.randn(P, 3, generator=g) * 0.5 - 3.0
    for s in states:
        s["grad"] = None
    opt, _ = R.build(opt_cls, states, device, torch.float32, step=5)
    if not state:
        opt.state.clear()
    stats = {"xyz_gradient_accum": torch.rand(P, 1, generator=g).to(device), "denom": torch.ones(P, 1).to(device),
             "max_radii2D": torch.rand(P, generator=g).to(device)}
    return opt, stats
