"""The MCMC strategy on the GPU (csrc/mcmc.hip): ``compute_relocation``, ``GaussianBag.relocate`` / ``add_new`` / ``mcmc_noise`` against
the plain-PyTorch restatement (tests/mcmc_reference.py) on the CPU, from the same fp32 state and the same draws.  Everything copied,
kept or zeroed must be equal bit for bit; the computed values (new opacity and scaling, the noise step) obey the yardstick
err(kernel) <= 2 * err(restatement in fp32) against the restatement in fp64 (mcmc_reference.assert_yardstick), both errors printed.

The kernels evaluate these values in double and round once, so their error is the rounding of the fp32 result; the figures
measured on an MI355X are in profiles/mcmc/NOTES.md."""
import math

import pytest
import torch

import adam_reference as R
import densify_reference as D
import mcmc_reference as M
from bags_raster import GaussianAdam, compute_relocation, relocation_binoms
from bags_raster.gaussians import GaussianBag

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEAF = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}
SIZES = (1, 64, 65, 257, 4099)
OPTS = {"GaussianAdam": GaussianAdam, "torch.optim.Adam": torch.optim.Adam}


# ---------------------------------------------------------------------------------------------------------------- compute_relocation
@pytest.mark.parametrize("P", [1, 63, 64, 65, 1000])
def test_compute_relocation(P):
    o, s, N = M.relocation_inputs(P, P)
    ref32, ref64 = M.compute_relocation(o, s, N), M.compute_relocation(o.double(), s.double(), N)
    n_dev = N.to(DEV)
    got = compute_relocation(o.to(DEV), s.to(DEV), n_dev, relocation_binoms(51, DEV), 51)
    assert torch.equal(n_dev.cpu(), N)                                                # clamped on read
    assert got[0].shape == (P,) and got[1].shape == (P, 3) and got[0].dtype == got[1].dtype == torch.float32
    rel32 = torch.maximum(((ref32[1].double() - ref64[1]).abs() / ref64[1].abs()).max(dim=1).values, (ref32[0].double() - ref64[0]).abs() / ref64[0].abs())
    big = N.clamp(1, 50) > 8
    rows = ~big | (rel32 < 1e-3)          # N <= 8: every row; larger N: where the fp32 statement itself is within 1e-3 of fp64
    if big.any():
        share = (rel32[big] < 1e-3).float().mean().item()
        print(f"MCMC compute_relocation P={P}: {share:.3f} of the rows with N > 8 qualify")
        assert share >= 0.9
    M.assert_yardstick(f"compute_relocation/P={P}/opacity", got[0].cpu()[rows], ref32[0][rows], ref64[0][rows])
    M.assert_yardstick(f"compute_relocation/P={P}/scale", got[1].cpu()[rows], ref32[1][rows], ref64[1][rows])
    # int64 counts and a (P,1) opacity, as the published caller passes them
    again = compute_relocation(o.to(DEV).reshape(P, 1), s.to(DEV), N.long().to(DEV), relocation_binoms(51, DEV), 51)
    assert again[0].shape == (P, 1) and torch.equal(again[0].reshape(-1), got[0]) and torch.equal(again[1], got[1])


def test_the_stub_is_real():
    """``diff_gaussian_rasterization.compute_relocation``, which utils/reloc_utils.py imports, computes: on the parent commit it raised."""
    import diff_gaussian_rasterization as dgr
    o, s, N = M.relocation_inputs(200, 7)
    N = N.clamp(1, 8)
    ref32, ref64 = M.compute_relocation(o, s, N), M.compute_relocation(o.double(), s.double(), N)
    got = dgr.compute_relocation(o.to(DEV), s.to(DEV), N.to(DEV), relocation_binoms(51, DEV), 51)
    M.assert_yardstick("stub/opacity", got[0].cpu(), ref32[0], ref64[0])
    M.assert_yardstick("stub/scale", got[1].cpu(), ref32[1], ref64[1])
    assert (got[0].cpu() <= o).all() and (got[1].cpu() <= s).all()


# ---------------------------------------------------------------------------------------------------------------- relocate, add_new
def _bag_of(opt, stats, deg):
    bag = GaussianBag(deg)
    for n, q in D.params(opt).items():
        setattr(bag, LEAF[n], q)
    bag.xyz_gradient_accum, bag.denom, bag.max_radii2D = stats["xyz_gradient_accum"], stats["denom"], stats["max_radii2D"]
    bag.active_sh_degree = deg
    return bag


def _case(P, seed, opt_name, deg, state):
    opt, stats = M.make_case(P, seed, OPTS[opt_name], DEV, sh_degree=deg, state=state)
    return opt, _bag_of(opt, stats, deg)


def _state(opt, p):
    st = opt.state.get(p, None)
    return st if st is not None and "exp_avg" in st else None


def _flat(opt):
    """Everything a call may touch, on the CPU: per group the parameter and, with state, both moments."""
    out = {}
    for n, q in D.params(opt).items():
        out[n] = q.detach().cpu().clone()
        st = _state(opt, q)
        if st is not None:
            out[n + ".exp_avg"], out[n + ".exp_avg_sq"] = st["exp_avg"].cpu().clone(), st["exp_avg_sq"].cpu().clone()
    return out


def _changed(before, after, P):
    rows = torch.zeros(P, dtype=torch.bool)
    for k in before:
        if before[k].numel():
            rows |= (before[k][:P] != after[k][:P]).reshape(P, -1).any(dim=1)
    return rows


def _draw(bag, rows, n, seed):
    """The draw the wrappers document: torch.multinomial over the opacities of ``rows`` under a generator seeded ``seed``."""
    p = torch.sigmoid(bag._opacity.detach()[rows, 0])
    return rows[torch.multinomial(p / p.sum(), n, replacement=True, generator=torch.Generator(device=DEV).manual_seed(seed))]


def _dead_patterns(P):
    every = torch.zeros(P, dtype=torch.bool)
    every[::2] = True
    one = torch.ones(P, dtype=torch.bool)
    one[P // 2] = False
    third = torch.zeros(P, dtype=torch.bool)
    third[: P // 3] = True
    return {"none": torch.zeros(P, dtype=torch.bool), "all": torch.ones(P, dtype=torch.bool), "one_alive": one, "every_second": every, "duplicates": third}


def _compare_values(label, got, ref32, ref64, rows):
    """New opacity and scaling of ``rows`` against the yardstick; elsewhere the three must agree bit for bit."""
    for n in ("opacity", "scaling"):
        assert torch.equal(got[n][~rows], ref32[n][~rows]), (label, n)
        if int(rows.sum()):
            M.assert_yardstick(f"{label}/{n}", got[n][rows], ref32[n][rows], ref64[n][rows])


@pytest.mark.parametrize("state", [True, False], ids=["state", "stateless"])
@pytest.mark.parametrize("opt_name", list(OPTS))
@pytest.mark.parametrize("deg", [0, 3])
@pytest.mark.parametrize("P", SIZES)
def test_relocate(P, deg, opt_name, state):
    for pattern, mask in _dead_patterns(P).items():
        label = f"relocate/P={P}/{pattern}"
        opt, bag = _case(P, P + deg, opt_name, deg, state)
        ref32, ref64 = D.clone_optimizer(opt), D.clone_optimizer(opt, dtype=torch.float64)
        before = _flat(opt)
        steps = {n: None if _state(opt, q) is None else float(_state(opt, q)["step"]) for n, q in D.params(opt).items()}
        leaves = list(bag.leaves())
        dead, alive = mask.nonzero().reshape(-1).to(DEV), (~mask).nonzero().reshape(-1).to(DEV)
        n_dead = int(dead.numel())
        if pattern == "duplicates" and n_dead and int(alive.numel()):
            sampled = alive[torch.arange(n_dead, device=DEV) % min(2, int(alive.numel()))]      # one or two sources for every dead row
            given = dict(sampled=sampled.int() if P % 2 else sampled)
        elif n_dead and int(alive.numel()):
            sampled = _draw(bag, alive, n_dead, seed=P)
            given = dict(generator=torch.Generator(device=DEV).manual_seed(P))
        else:
            sampled, given = torch.zeros(0, dtype=torch.long, device=DEV), {}
        out = bag.relocate(opt, mask.to(DEV), **given)
        a, b = M.relocate(ref32, mask, sampled.cpu().long()), M.relocate(ref64, mask, sampled.cpu().long())
        assert out == a == b, (label, out, a, b)
        if pattern == "one_alive" and P >= 64:
            assert out == {"dead": P - 1, "sources": 1}                               # P - 1 > 50 copies: the count is clamped to 50
        assert all(x is y for x, y in zip(bag.leaves(), leaves)) and all(getattr(bag, LEAF[g["name"]]) is g["params"][0] for g in opt.param_groups)      # in place
        got, want32, want64 = _flat(opt), _flat(ref32), _flat(ref64)
        assert got.keys() == want32.keys()
        touched = torch.zeros(P, dtype=torch.bool)
        if a["sources"]:
            touched[mask] = True
            touched[sampled.cpu().long()] = True
        for k in got:
            if k not in ("opacity", "scaling"):
                assert torch.equal(got[k], want32[k]), (label, k)                     # copied values, zeroed moments, untouched rows
        _compare_values(label, got, want32, want64, touched)
        if a["sources"]:
            assert torch.equal(got["opacity"][mask], got["opacity"][sampled.cpu().long()]) and torch.equal(got["scaling"][mask], got["scaling"][sampled.cpu().long()])
        assert torch.equal(_changed(before, got, P), _changed(before, want32, P)) and not _changed(before, got, P)[~touched].any(), label
        for n, q in D.params(opt).items():
            st = _state(opt, q)
            assert (st is None) == (steps[n] is None) and (st is None or float(st["step"]) == steps[n]), (label, n)
        assert len(opt.state) == (6 if state else 0)
        # a second run from the same state: the same bits
        opt2, bag2 = _case(P, P + deg, opt_name, deg, state)
        bag2.relocate(opt2, mask.to(DEV), **(dict(given, generator=torch.Generator(device=DEV).manual_seed(P)) if "generator" in given else given))
        again = _flat(opt2)
        assert all(torch.equal(got[k], again[k]) for k in got), label


@pytest.mark.parametrize("deg,opt_name,state", [(3, "GaussianAdam", True), (0, "GaussianAdam", False), (3, "torch.optim.Adam", True), (0, "torch.optim.Adam", True)])
@pytest.mark.parametrize("P", SIZES)
def test_add_new(P, deg, opt_name, state):
    room = int(1.05 * P) - P
    caps = {"below": max(P - 1, 0), "equal": P, "between": P + max(room // 2, 1) if room >= 2 else P + room, "above": 10 * P + 7}
    for name, cap in caps.items():
        label = f"add_new/P={P}/{name}"
        opt, bag = _case(P, 3 * P + deg, opt_name, deg, state)
        ref32, ref64 = D.clone_optimizer(opt), D.clone_optimizer(opt, dtype=torch.float64)
        before = _flat(opt)
        old = list(bag.leaves())
        steps = {n: None if _state(opt, q) is None else float(_state(opt, q)["step"]) for n, q in D.params(opt).items()}
        A = max(0, min(cap, int(1.05 * P)) - P)
        assert (A == 0) == (name in ("below", "equal") or room == 0) and (name != "between" or A <= room)
        every = torch.arange(P, device=DEV)
        if name == "between" and A:
            sampled = every[torch.arange(A, device=DEV) % min(2, P)]                  # duplicates
            given = dict(sampled=sampled)
        else:
            sampled = _draw(bag, every, A, seed=P + 1) if A else torch.zeros(0, dtype=torch.long, device=DEV)
            given = dict(generator=torch.Generator(device=DEV).manual_seed(P + 1))
        out = bag.add_new(opt, cap, **given)
        a, b = M.add_new(ref32, cap, sampled.cpu()), M.add_new(ref64, cap, sampled.cpu())
        assert out == {"added": A, "P_new": P + A} and (a["added"], a["P_new"]) == (A, P + A) == (b["added"], b["P_new"]), label
        if A == 0:
            assert all(x is y for x, y in zip(bag.leaves(), old)) and all(torch.equal(v, before[k]) for k, v in _flat(opt).items())
            assert bag.denom.shape == (P, 1) and bag.denom.sum().item() == P          # the statistics too are left alone
            continue
        got, want32, want64 = _flat(opt), _flat(ref32), _flat(ref64)
        assert got.keys() == want32.keys()
        for n, g in zip(R.NAMES, opt.param_groups):
            q = g["params"][0]
            assert g["name"] == n and q is getattr(bag, LEAF[n]) and q.is_leaf and q.requires_grad and q.grad is None and q.is_cuda and q.shape[0] == P + A, (label, n)
            st = _state(opt, q)
            assert (st is None) == (steps[n] is None), (label, n)
            if st is not None:
                assert float(st["step"]) == steps[n] and not st["step"].is_cuda and st["exp_avg"].shape == q.shape == st["exp_avg_sq"].shape
                assert st["exp_avg"][P:].abs().max().item() == 0.0 and st["exp_avg_sq"][P:].abs().max().item() == 0.0 if q.numel() else True
        assert len(opt.state) == (6 if state else 0) and all(all(q is not k for k in opt.state) for q in old)        # the old parameters' entries are gone
        touched = torch.zeros(P + A, dtype=torch.bool)
        touched[sampled.cpu()] = True
        touched[P:] = True
        for k in got:
            assert got[k].shape == want32[k].shape, (label, k)
            if k not in ("opacity", "scaling"):
                assert torch.equal(got[k], want32[k]), (label, k)
        _compare_values(label, got, want32, want64, touched)
        assert torch.equal(got["opacity"][P:], got["opacity"][sampled.cpu()]) and torch.equal(got["scaling"][P:], got["scaling"][sampled.cpu()])
        assert torch.equal(_changed(before, got, P), _changed(before, want32, P)) and not _changed(before, got, P)[~touched[:P]].any(), label
        for t, shape in ((bag.xyz_gradient_accum, (P + A, 1)), (bag.denom, (P + A, 1)), (bag.max_radii2D, (P + A,))):
            assert tuple(t.shape) == shape and t.is_cuda and t.abs().max().item() == 0.0, label


def test_add_new_then_step_and_render():
    """After the call the bag's leaves are the optimizer's parameters; a rasterizer forward + backward and a GaussianAdam step run
    on the grown set, and a relocation of its most transparent rows after that."""
    from bags_raster.render import render, PipelineParams
    from bags_raster.synth import sphere_views
    opt, bag = _case(1001, 4, "GaussianAdam", 3, True)
    with torch.no_grad():
        bag._xyz.mul_(0.2)                                         # in front of the camera
    out = bag.add_new(opt, 5000)
    assert out == {"added": 50, "P_new": 1051}
    assert [g["params"][0] for g in opt.param_groups] == [getattr(bag, LEAF[n]) for n in R.NAMES]
    cam = sphere_views(1, 96, 64, device=DEV)[0]
    res = render(cam, bag, PipelineParams(), torch.zeros(3, device=DEV), 0.0, None, hybrid=False)
    res["render"].sum().backward()
    assert all(t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad).all() for t in bag.leaves())
    assert res["radii"].numel() == 1051 and int((res["radii"] > 0).sum()) > 0
    before = bag._features_dc.detach().clone()
    opt.step(stats=(bag, res["viewspace_points"], res["radii"]))
    assert not torch.equal(before, bag._features_dc.detach()) and bag.denom.sum().item() > 0
    assert all(float(opt.state[q]["step"]) == 6.0 and opt.state[q]["exp_avg"].shape == q.shape for q in bag.leaves())
    dead = (torch.sigmoid(bag._opacity.detach()) <= 0.05).reshape(-1)
    moved = bag.relocate(opt, dead, generator=torch.Generator(device=DEV).manual_seed(1))
    assert moved["dead"] == int(dead.sum()) > 0 and 0 < moved["sources"] <= moved["dead"]
    assert torch.sigmoid(bag._opacity.detach())[dead].min().item() >= 0.005 * (1 - 1e-6)       # a relocated row is at least min_opacity
    res = render(cam, bag, PipelineParams(), torch.zeros(3, device=DEV), 0.0, None, hybrid=False)
    assert torch.isfinite(res["render"]).all()


# ---------------------------------------------------------------------------------------------------------------- mcmc_noise
def _noise_bag(P, seed):
    """Opacities on both sides of the gate (1 - o around x0 = 0.995: o from 0.0005 to 0.02), a few opaque rows, anisotropic scales."""
    g = torch.Generator().manual_seed(seed)
    o = torch.exp(math.log(0.0005) + (math.log(0.02) - math.log(0.0005)) * torch.rand(P, 1, generator=g))
    o[torch.rand(P, generator=g) < 0.2] = 0.9
    scene = {"means3D": torch.randn(P, 3, generator=g), "shs": torch.zeros(P, 1, 3), "scales": torch.exp(torch.randn(P, 3, generator=g) * 0.7 - 1.0),
             "rotations": torch.randn(P, 4, generator=g), "opacities": o}
    return GaussianBag.from_activated(scene, 0, device=DEV), torch.randn(P, 3, generator=g)


@pytest.mark.parametrize("P", [1, 65, 1000])
def test_noise_step_with_given_noise(P):
    bag, z = _noise_bag(P, P)
    raw = [t.detach().cpu() for t in (bag._xyz, bag._opacity, bag._scaling, bag._rotation)]
    gate = M.gate(raw[1].double())
    if P > 1:
        assert gate.min().item() < 0.2 and gate.max().item() > 0.55               # both sides of the gate are there
    for scale, modifier in ((0.8, 1.0), (0.05, 1.7)):
        fresh, _ = _noise_bag(P, P)
        ref32 = M.mcmc_noise(*raw, scale, z, scaling_modifier=modifier)
        ref64 = M.mcmc_noise(*[t.double() for t in raw], scale, z.double(), scaling_modifier=modifier)
        others = [t.detach().clone() for t in (fresh._opacity, fresh._scaling, fresh._rotation)]
        assert fresh.mcmc_noise(scale, noise=z.to(DEV), scaling_modifier=modifier) is None
        assert fresh._xyz.requires_grad and fresh._xyz.is_leaf
        M.assert_yardstick(f"mcmc_noise/P={P}/scale={scale}", fresh._xyz.detach().cpu(), ref32, ref64)
        assert all(torch.equal(a, b.detach()) for a, b in zip(others, (fresh._opacity, fresh._scaling, fresh._rotation)))
        if P > 1:
            assert not torch.equal(fresh._xyz.detach().cpu(), raw[0])
    bag.mcmc_noise(0.0, noise=z.to(DEV))
    assert torch.equal(bag._xyz.detach().cpu(), raw[0])                            # scale = 0: bit for bit
    bag.mcmc_noise(0.0, seed=3)
    assert torch.equal(bag._xyz.detach().cpu(), raw[0])


def test_noise_step_with_the_generator():
    half, P = 100_000, 120_000                   # 100 000 rows of unit covariance and open gate, then 20 000 with the gate closed
    g = torch.Generator().manual_seed(9)
    o = torch.cat((torch.full((half, 1), 1e-4), 0.5 + 0.4999 * torch.rand(P - half, 1, generator=g)))      # open gate | opacity up to 1
    scales = torch.cat((torch.ones(half, 3), torch.exp(torch.randn(P - half, 3, generator=g) * 0.5)))        # unit covariance | any
    xyz = torch.cat((torch.zeros(half, 3), torch.randn(P - half, 3, generator=g)))
    scene = {"means3D": xyz, "shs": torch.zeros(P, 1, 3), "scales": scales, "rotations": torch.randn(P, 4, generator=g), "opacities": o}

    def run(seed):
        bag = GaussianBag.from_activated(scene, 0, device=DEV)
        if seed is None:
            bag.mcmc_noise(0.5)
        else:
            bag.mcmc_noise(0.5, seed=seed)
        return bag._xyz.detach().cpu()
    a, b, c = run(2024), run(2024), run(2025)
    assert torch.equal(a, b)                                                       # one seed: the same bits
    assert not (a[:half] == c[:half]).all(dim=1).any()                             # another seed: every open row moved elsewhere
    torch.manual_seed(5)
    d = run(None)
    torch.manual_seed(5)
    e = run(None)
    assert torch.equal(d, e) and not torch.equal(d[:half], a[:half])               # seed=None: torch's CPU generator governs
    # unit covariance, open gate: step / (g * scale) is z itself
    raw_o = torch.log(o[:half] / (1 - o[:half]))
    zs = a[:half].double() / (M.gate(raw_o.double()) * 0.5)
    assert zs.shape == (100_000, 3)
    n = zs.numel()
    mean, var = zs.mean().item(), zs.var().item()
    print(f"MCMC generator: rows {zs.shape[0]} normals {n} mean {mean:.3e} (bound {5 / math.sqrt(n):.3e}) var - 1 {var - 1:.3e} (bound {5 * math.sqrt(2 / n):.3e}) max |z| {zs.abs().max().item():.3f}")
    assert abs(mean) <= 5 / math.sqrt(n) and abs(var - 1) <= 5 * math.sqrt(2 / n)
    for axis in range(3):
        assert abs(zs[:, axis].mean().item()) <= 5 / math.sqrt(n / 3) and abs(zs[:, axis].var().item() - 1) <= 5 * math.sqrt(6 / n)
    # opacity near 1: the step is at most what the fp32 statement gives at the same gate for the largest normal the generator can
    # produce (Box-Muller on 32-bit uniforms: |z| <= sqrt(2 * 33 * ln 2) < 7 per axis).  With opacity >= 0.5 that gate is at most
    # exp(-49.5) = 3e-22 and the bound of the order of 1e-19: far below half an ulp of these xyz, so the step is lost in the fp32 sum and
    # the rows stay where they are (which the bound allows, and more it does not).
    raw = [t[half:] for t in (xyz, torch.log(o / (1 - o)), torch.log(scales), scene["rotations"])]
    L = D.build_rotation(raw[3]) * torch.exp(raw[2]).unsqueeze(1)
    bound = torch.bmm((L @ L.transpose(1, 2)).abs(), (7.0 * M.gate(raw[1]) * 0.5).expand(-1, 3).unsqueeze(-1)).squeeze(-1)
    moved = (a[half:] - xyz[half:]).abs()
    print(f"MCMC closed gate: max bound {bound.max().item():.3e} max move {moved.max().item():.3e}")
    assert (moved <= bound).all() and bound.max().item() < 1e-15
