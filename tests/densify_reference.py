"""Reference side of the densification tests: ``GaussianModel.densify_and_prune`` and ``reset_opacity`` restated in plain PyTorch
(the published 3DGS method, scene/gaussian_model.py:393-447: clone, split, prune, each with its optimizer surgery), on any device
and in fp32 or fp64, built on the pinned ``adam_reference.cat_tensors_to_optimizer`` / ``prune_optimizer``.  Never the code under
test.  Also the generator of the test inputs, whose two properties (every class populated, no row near a threshold) are checked
on the CPU by tests/test_densify_cpu.py.

The optimizer holds the six groups of ``adam_reference.NAMES`` in that order, one parameter each; ``stats`` is a dict of
``xyz_gradient_accum (P,1)``, ``denom (P,1)``, ``max_radii2D (P)``.  ``torch.normal(0, stds)`` of the published code is
``stds * z`` with ``z = noise[source row, child]``, ``noise`` of shape ``(P, N, 3)``.
"""
import torch

import adam_reference as R

RULE = dict(max_grad=0.0002, min_opacity=0.005, extent=5.0, max_screen_size=20, percent_dense=0.01)
KEPT, CLONE, CHILD = 0, 1, 2          # provenance kinds; child k is CHILD + k


def params(opt):
    return {g["name"]: g["params"][0] for g in opt.param_groups}


def build_rotation(r):
    """utils/general_utils.py:129-152"""
    q = r / torch.sqrt((r * r).sum(dim=1, keepdim=True))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=1).view(-1, 3, 3)


# tools/bench_densify.py switches both off: the margins and the provenance map (with the pre-densify radii that ride along) are the
# tests' bookkeeping, no part of the published method.  Without PROVENANCE the result holds no kept count and no map, and
# screen_size="pre_densify" is not available.
MARGINS = True
PROVENANCE = True


def _margin(values, threshold):
    """Smallest |v - t| / |t| over the values a test compares with ``threshold``."""
    if values.numel() == 0 or not MARGINS:
        return float("inf")
    d = (values.detach().double() - float(threshold)).abs() / abs(float(threshold))
    return d.min().item()


def densify_and_prune(opt, stats, max_grad, min_opacity, extent, max_screen_size, percent_dense=0.01, N=2, noise=None,
                      screen_size="published"):
    """The published sequence on ``opt`` (modified in place, as the reference modifies its optimizer).  Returns a dict: the counts
    ``kept / clones / split / pruned / P_new``, ``provenance`` (P_new, 2) int64 = (source row, kind), the new ``stats`` (zeros of
    the new size) and ``margin``: the smallest relative distance of any tested value from the threshold it was tested against."""
    assert screen_size in ("published", "pre_densify")
    track = PROVENANCE
    assert track or screen_size == "published"
    p = params(opt)
    dev, dt = p["xyz"].device, p["xyz"].dtype
    P = p["xyz"].shape[0]
    thr = percent_dense * extent
    grads = stats["xyz_gradient_accum"].to(dev, dt) / stats["denom"].to(dev, dt)
    grads[grads.isnan()] = 0.0
    if track:
        prov = torch.stack((torch.arange(P, device=dev), torch.zeros(P, dtype=torch.int64, device=dev)), dim=1)
        radii_pre = stats["max_radii2D"].to(dev, dt).clone()
    margins = [_margin(grads.abs()[grads.abs() != float("inf")], max_grad)] if max_grad != 0 else []

    # ---- densify_and_clone (:430-445) + densification_postfix
    scal = torch.exp(p["scaling"].detach()).max(dim=1).values
    margins.append(_margin(scal, thr))
    sel = (torch.norm(grads, dim=-1) >= max_grad) & (scal <= thr)
    n_clone = int(sel.sum())
    R.cat_tensors_to_optimizer(opt, [p[n].detach()[sel] for n in R.NAMES])
    p = params(opt)
    if track:
        prov = torch.cat((prov, torch.stack((prov[sel, 0], torch.full((n_clone,), CLONE, dtype=torch.int64, device=dev)), dim=1)))
        radii_pre = torch.cat((radii_pre, torch.zeros(n_clone, device=dev, dtype=dt)))

    # ---- densify_and_split (:405-428): the gradient padded with zeros, so a clone never splits
    n_now = P + n_clone
    padded = torch.zeros(n_now, device=dev, dtype=dt)
    padded[:P] = grads.reshape(-1)
    scal3 = torch.exp(p["scaling"].detach())
    sel2 = (padded.abs() >= max_grad) & (scal3.max(dim=1).values > thr)
    S = int(sel2.sum())
    src = prov[sel2, 0] if track else sel2[:P].nonzero().reshape(-1)          # a clone never splits: the selected rows are originals
    if noise is None:
        z = torch.zeros(N * S, 3, device=dev, dtype=dt)
    else:
        z = noise.to(dev, dt)[src].permute(1, 0, 2).reshape(N * S, 3)
    stds = scal3[sel2].repeat(N, 1)
    samples = stds * z
    rots = build_rotation(p["rotation"].detach()[sel2]).repeat(N, 1, 1)
    ext = {"xyz": torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + p["xyz"].detach()[sel2].repeat(N, 1),
           "scaling": torch.log(scal3[sel2].repeat(N, 1) / (0.8 * N)),
           "rotation": p["rotation"].detach()[sel2].repeat(N, 1),
           "f_dc": p["f_dc"].detach()[sel2].repeat(N, 1, 1),
           "f_rest": p["f_rest"].detach()[sel2].repeat(N, 1, 1),
           "opacity": p["opacity"].detach()[sel2].repeat(N, 1)}
    R.cat_tensors_to_optimizer(opt, [ext[n] for n in R.NAMES])
    keep = ~torch.cat((sel2, torch.zeros(N * S, dtype=torch.bool, device=dev)))
    R.prune_optimizer(opt, keep)
    if track:
        kinds = torch.arange(N, device=dev).repeat_interleave(S) + CHILD
        prov = torch.cat((prov, torch.stack((src.repeat(N), kinds), dim=1)))
        radii_pre = torch.cat((radii_pre, torch.zeros(N * S, device=dev, dtype=dt)))
        prov, radii_pre = prov[keep], radii_pre[keep]
    p = params(opt)

    # ---- prune (:393-403): opacity, and with max_screen_size the two size tests
    o = torch.sigmoid(p["opacity"].detach()).reshape(-1)
    margins.append(_margin(o, min_opacity) if min_opacity != 0 else float("inf"))
    mask = o < min_opacity
    if max_screen_size is not None:
        radii = radii_pre if screen_size == "pre_densify" else torch.zeros_like(o)      # published: zeroed by the postfix
        s_now = torch.exp(p["scaling"].detach()).max(dim=1).values
        margins += [_margin(radii, max_screen_size), _margin(s_now, 0.1 * extent)]
        mask = mask | (radii > max_screen_size) | (s_now > 0.1 * extent)
    n_pruned = int(mask.sum())
    R.prune_optimizer(opt, ~mask)
    P_new = o.shape[0] - n_pruned
    if track:
        prov = prov[~mask]
        assert prov.shape[0] == P_new
    new_stats = {"xyz_gradient_accum": torch.zeros(P_new, 1, device=dev, dtype=dt), "denom": torch.zeros(P_new, 1, device=dev, dtype=dt),
                 "max_radii2D": torch.zeros(P_new, device=dev, dtype=dt)}
    return {"kept": int((prov[:, 1] == KEPT).sum()) if track else None, "clones": n_clone, "split": S, "pruned": n_pruned, "P_new": P_new,
            "provenance": prov.cpu() if track else None, "stats": new_stats, "margin": min(margins)}


def reset_opacity(opt):
    """GaussianModel.reset_opacity + replace_tensor_to_optimizer: a new parameter, both moments zero."""
    group = [g for g in opt.param_groups if g["name"] == "opacity"][0]
    old = group["params"][0]
    x = torch.min(torch.sigmoid(old.detach()), torch.ones_like(old) * 0.01)
    new = torch.nn.Parameter(torch.log(x / (1 - x)).requires_grad_(True))
    stored = opt.state.get(old, None)
    if stored is not None:
        stored["exp_avg"] = torch.zeros_like(new)
        stored["exp_avg_sq"] = torch.zeros_like(new)
        del opt.state[old]
        opt.state[new] = stored
    group["params"][0] = new
    return new


# ---------------------------------------------------------------------------------------------------------- test inputs
def make_inputs(P, seed):
    """fp32 CPU inputs for RULE in which every class is populated and no tested value is near its threshold.  Per row, drawn
    independently: selected (|g| in [2, 10] max_grad, else [0, 0.5] max_grad or 0 / 0), scale class small ([0.2, 0.8] thr), large
    ([1.5, 4] thr: a split candidate, children and itself below 0.1 extent), over ([1.15, 1.4] x 0.1 extent: itself above, its two
    or three children below) or huge ([3, 5] x 0.1 extent: itself and its children above), opacity low ([0.0003, 0.003]) or high ([0.02, 0.99]), radius small ([0, 12]) or big ([30, 100]).
    Returns (states for adam_reference.build with zero moments, stats, [gradients of three Adam steps])."""
    g = torch.Generator().manual_seed(seed)
    u = lambda lo, hi: lo + (hi - lo) * torch.rand(P, generator=g)
    r = RULE
    thr, big = r["percent_dense"] * r["extent"], 0.1 * r["extent"]
    selected = torch.rand(P, generator=g) < 0.5
    cls = torch.rand(P, generator=g)
    smax = torch.where(cls < 0.45, u(0.2, 0.8) * thr, torch.where(cls < 0.8, u(1.5, 4.0) * thr, torch.where(cls < 0.9, u(1.15, 1.4) * big, u(3.0, 5.0) * big)))
    scales = smax[:, None] * (0.1 + 0.9 * torch.rand(P, 3, generator=g))
    scales[torch.arange(P), torch.randint(0, 3, (P,), generator=g)] = smax
    opac = torch.where(torch.rand(P, generator=g) < 0.15, u(0.0003, 0.003), u(0.02, 0.99))
    radii = torch.where(torch.rand(P, generator=g) < 0.1, u(30, 100), u(0, 12)).round()
    denom = torch.randint(1, 40, (P,), generator=g).float()
    mean_grad = torch.where(selected, u(2.0, 10.0), u(0.0, 0.5)) * r["max_grad"]
    accum = mean_grad * denom
    unseen = torch.rand(P, generator=g) < 0.05                    # never visible: 0 / 0 = NaN -> 0
    denom[unseen] = 0.0
    accum[unseen] = 0.0
    tensors = {"xyz": torch.randn(P, 3, generator=g) * 2.0, "f_dc": torch.randn(P, 1, 3, generator=g), "f_rest": torch.randn(P, 15, 3, generator=g) * 0.1,
               "opacity": torch.log(opac / (1 - opac)).reshape(P, 1), "scaling": torch.log(scales), "rotation": torch.randn(P, 4, generator=g)}
    states = [dict(param=tensors[n], grad=None, exp_avg=torch.zeros_like(tensors[n]), exp_avg_sq=torch.zeros_like(tensors[n])) for n in R.NAMES]
    stats = {"xyz_gradient_accum": accum.reshape(P, 1), "denom": denom.reshape(P, 1), "max_radii2D": radii}
    grads = [[torch.randn(tensors[n].shape, generator=g) * 0.01 for n in R.NAMES] for _ in range(3)]
    return states, stats, grads


def make_case(P, seed, opt_cls=torch.optim.Adam, device="cpu", steps=3):
    """An optimizer of ``opt_cls`` over make_inputs(P, seed) after ``steps`` real Adam steps (so moments and ``step`` are real), the
    statistics on ``device``, and the noise (P, 3, 3) of up to three children, fp32 on the CPU."""
    states, stats, grads = make_inputs(P, seed)
    opt, ps = R.build(opt_cls, states, device, torch.float32, step=0)
    for k in range(steps):
        for p, gr in zip(ps, grads[k]):
            p.grad = gr.to(device)
        opt.step()
    for p in ps:
        p.grad = None
    noise = torch.randn(P, 3, 3, generator=torch.Generator().manual_seed(seed + 1000))
    return opt, {k: v.to(device) for k, v in stats.items()}, noise


def clone_optimizer(opt, device="cpu", dtype=torch.float32, opt_cls=torch.optim.Adam):
    """A torch.optim.Adam on ``device`` / ``dtype`` with copies of the parameters and state of ``opt`` (any device)."""
    new_params = [torch.nn.Parameter(g["params"][0].detach().to(device, dtype).clone()) for g in opt.param_groups]
    new = opt_cls([{"params": [q], "lr": g["lr"], "name": g["name"]} for q, g in zip(new_params, opt.param_groups)], lr=0.0, betas=R.BETAS, eps=R.EPS)
    for q, g in zip(new_params, opt.param_groups):
        st = opt.state.get(g["params"][0], None)
        if st is not None and "exp_avg" in st:
            new.state[q] = {"step": st["step"].detach().cpu().clone(), "exp_avg": st["exp_avg"].detach().to(device, dtype).clone(),
                            "exp_avg_sq": st["exp_avg_sq"].detach().to(device, dtype).clone()}
    return new
