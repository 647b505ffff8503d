"""Reference side of the GaussianAdam tests: ``torch.optim.Adam`` in float64 on the CPU, the error measure, and the rule that
turns PyTorch's own fp32 error into the bound (no tolerance is fixed in advance).

    err(x) = max |x - ref64| / (eps32 * (|ref64| + mean |ref64|))
    required: err(kernel) <= 2 * err(torch fp32) + 1

The factor 2 allows a different but equally valid rounding order (FMA contraction, the lerp form); the + 1 a tie on the last
rounding.  ``ref64`` is always torch.optim.Adam(float64) from the same fp32 state and gradients, upcast; never GaussianAdam.
"""
import math

import torch

EPS32 = 2.0 ** -23
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
SHAPES = ((3,), (1, 3), (15, 3), (1,), (3,), (4,))          # per Gaussian: widths 3, 3, 45, 1, 3, 4 (scene/gaussian_model.py:192-210)
LRS = (0.00016, 0.0025, 0.0025 / 20.0, 0.05, 0.005, 0.001)  # the reference's training_setup rates (spatial_lr_scale = 1)
BETAS = (0.9, 0.999)
EPS = 1e-15
KEYS = ("param", "exp_avg", "exp_avg_sq")


def err(x: torch.Tensor, ref64: torch.Tensor) -> float:
    x = x.detach().to("cpu", torch.float64)
    ref = ref64.detach().to("cpu", torch.float64)
    assert x.shape == ref.shape, (x.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    d = (x - ref).abs()
    den = EPS32 * (ref.abs() + ref.abs().mean())
    return torch.where(d == 0, torch.zeros_like(d), d / den).max().item()       # NaN anywhere -> NaN -> every comparison fails


WORST = {}          # label family -> (err kernel, err torch fp32) with the largest err kernel seen in this process


def assert_rule(label: str, kernel: torch.Tensor, torch32: torch.Tensor, ref64: torch.Tensor) -> None:
    ek, et = err(kernel, ref64), err(torch32, ref64)
    print(f"ADAM_ERR {label}: kernel {ek:.4f} torch_fp32 {et:.4f} bound {2 * et + 1:.4f}")
    fam = label.split("/")[0]
    if fam not in WORST or not ek <= WORST[fam][0]:
        WORST[fam] = (ek, et)
    assert ek <= 2.0 * et + 1.0, f"{label}: err(kernel) = {ek:.4f} > 2 * err(torch fp32) + 1 = {2 * et + 1:.4f} (err(torch fp32) = {et:.4f})"


def random_state(P: int, seed: int, zero_rows: float = 0.25, shapes=SHAPES):
    """Per group a dict of fp32 CPU tensors: param, grad (a seeded share of all-zero rows), exp_avg, exp_avg_sq >= 0."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for shp in shapes:
        full = (P,) + tuple(shp)
        grad = torch.randn(full, generator=g) * 0.01
        dead = torch.rand(P, generator=g) < zero_rows
        grad[dead] = 0.0
        out.append(dict(param=torch.randn(full, generator=g) * 2.0, grad=grad, exp_avg=torch.randn(full, generator=g) * 0.01,
                        exp_avg_sq=torch.rand(full, generator=g) * 1e-4))
    return out


def param_groups(tensors, lrs=LRS, names=NAMES):
    return [{"params": [t], "lr": lr, "name": n} for t, lr, n in zip(tensors, lrs, names)]


def build(opt_cls, states, device, dtype, step: int = 0, lrs=LRS, names=NAMES, **kw):
    """An optimizer of ``opt_cls`` over copies of ``states`` (random_state) on ``device`` / ``dtype``, its state injected with
    ``step`` steps already counted (0: fresh state from the tensors all the same), gradients set where the state has one."""
    params = [torch.nn.Parameter(s["param"].to(device, dtype).clone()) for s in states]
    opt = opt_cls(param_groups(params, lrs, names), lr=0.0, betas=BETAS, eps=EPS, **kw)
    for p, s in zip(params, states):
        opt.state[p] = {"step": torch.tensor(float(step)), "exp_avg": s["exp_avg"].to(device, dtype).clone(),
                        "exp_avg_sq": s["exp_avg_sq"].to(device, dtype).clone()}
        p.grad = None if s.get("grad") is None else s["grad"].to(device, dtype).clone()
    return opt, params


def snapshot(opt, params):
    """[(param, exp_avg, exp_avg_sq, step)] per group, detached clones."""
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), float(opt.state[p]["step"]))
            for p in params]


def torch_adam_step(states, step: int, dtype, device="cpu", visible=None, lrs=LRS):
    """One torch.optim.Adam step (number ``step``, counted from 1) from ``states``; with ``visible`` (bool (P,)) the rows that
    are not visible keep their old param / exp_avg / exp_avg_sq: the masked form."""
    opt, params = build(torch.optim.Adam, states, device, dtype, step - 1, lrs)
    opt.step()
    out = snapshot(opt, params)
    if visible is not None:
        keep = ~visible.to(device)
        for (p, m, v, _), s in zip(out, states):
            if s.get("grad") is None:
                continue
            for new, old in ((p, s["param"]), (m, s["exp_avg"]), (v, s["exp_avg_sq"])):
                new[keep] = old.to(device, dtype)[keep]
    return out


def closed_form_step64(states, step: int, visible=None, lrs=LRS):
    """The update written out in float64 (the formula csrc/adam.hip implements), for checking torch_adam_step itself."""
    b1, b2 = BETAS
    out = []
    for s, lr in zip(states, lrs):
        p, m, v = (s[k].double() for k in KEYS)
        if s.get("grad") is None:
            out.append((p, m, v, float(step - 1)))
            continue
        g = s["grad"].double()
        m2 = m + (1 - b1) * (g - m)
        v2 = v * b2 + (1 - b2) * g * g
        p2 = p - lr / (1 - b1 ** step) * (m2 / (v2.sqrt() / math.sqrt(1 - b2 ** step) + EPS))
        if visible is not None:
            keep = ~visible
            p2[keep], m2[keep], v2[keep] = p[keep], m[keep], v[keep]
        out.append((p2, m2, v2, float(step)))
    return out


def cat_tensors_to_optimizer(opt, extensions):
    """GaussianModel.cat_tensors_to_optimizer (scene/gaussian_model.py:366-386): one new, longer nn.Parameter per group,
    moments extended with zeros, the state entry moved to the new parameter."""
    for group, ext in zip(opt.param_groups, extensions):
        old = group["params"][0]
        ext = ext.to(old.device, old.dtype)
        stored = opt.state.get(old, None)
        if stored is not None:
            stored["exp_avg"] = torch.cat((stored["exp_avg"], torch.zeros_like(ext)), dim=0)
            stored["exp_avg_sq"] = torch.cat((stored["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
            del opt.state[old]
            group["params"][0] = torch.nn.Parameter(torch.cat((old.detach(), ext), dim=0).requires_grad_(True))
            opt.state[group["params"][0]] = stored
        else:
            group["params"][0] = torch.nn.Parameter(torch.cat((old.detach(), ext), dim=0).requires_grad_(True))
    return [g["params"][0] for g in opt.param_groups]


def prune_optimizer(opt, mask):
    """GaussianModel._prune_optimizer (scene/gaussian_model.py:324-340): keep the rows of ``mask``."""
    for group in opt.param_groups:
        old = group["params"][0]
        mk = mask.to(old.device)
        stored = opt.state.get(old, None)
        if stored is not None:
            stored["exp_avg"] = stored["exp_avg"][mk]
            stored["exp_avg_sq"] = stored["exp_avg_sq"][mk]
            del opt.state[old]
            group["params"][0] = torch.nn.Parameter(old.detach()[mk].requires_grad_(True))
            opt.state[group["params"][0]] = stored
        else:
            group["params"][0] = torch.nn.Parameter(old.detach()[mk].requires_grad_(True))
    return [g["params"][0] for g in opt.param_groups]
