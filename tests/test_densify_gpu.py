"""GaussianBag.densify_and_prune / reset_opacity (csrc/densify.hip) against the plain-PyTorch restatement of the published method
(tests/densify_reference.py) on the CPU, from the same fp32 state and the same noise.  Decisions, order and every copied quantity
must be equal bit for bit; the computed ones (children's xyz and scaling, the reset opacity) obey the rule of tests/adam_reference.py:
err(kernel) <= 2 * err(restatement in fp32) + 1 against the restatement in fp64.  No row is excluded from any comparison: the
inputs keep every tested value away from its threshold, which each test asserts on the fp64 restatement before it compares."""
import math

import pytest
import torch

import adam_reference as R
import densify_reference as D
from bags_raster.gaussians import GaussianBag

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEAF = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}


def _bag_of(opt, stats, bag=None):
    bag = bag or GaussianBag(3)
    for n, q in D.params(opt).items():
        setattr(bag, LEAF[n], q)
    bag.xyz_gradient_accum, bag.denom, bag.max_radii2D = stats["xyz_gradient_accum"], stats["denom"], stats["max_radii2D"]
    bag.active_sh_degree = 3
    return bag


def _case(P, seed, opt_cls=None, steps=3):
    from bags_raster import GaussianAdam
    opt, stats, noise = D.make_case(P, seed, opt_cls or GaussianAdam, DEV, steps=steps)
    return opt, _bag_of(opt, stats), stats, noise


def _state(opt, p):
    st = opt.state.get(p, None)
    return st if st is not None and "exp_avg" in st else None


def _compare(label, opt, bag, stats, noise, N=2, mode="published", rule=D.RULE, populated=True, near=True):
    """Runs the fused call on (opt, bag) and the restatement (fp32 and fp64, CPU) on copies of the same state; asserts everything
    the two must share.  Returns (fused result, fp64 restatement result)."""
    P = bag._xyz.shape[0]
    steps = {n: None if _state(opt, q) is None else float(_state(opt, q)["step"]) for n, q in D.params(opt).items()}
    ref32, ref64 = D.clone_optimizer(opt), D.clone_optimizer(opt, dtype=torch.float64)
    cpu_stats = {k: v.cpu() for k, v in stats.items()}
    z = noise[:, :N].contiguous()
    a = D.densify_and_prune(ref32, cpu_stats, noise=z, N=N, screen_size=mode, **rule)
    b = D.densify_and_prune(ref64, cpu_stats, noise=z, N=N, screen_size=mode, **rule)
    print(f"DENSIFY {label}: P {P} -> {b['P_new']} kept {b['kept']} clones {b['clones']} split {b['split']} pruned {b['pruned']} margin {b['margin']:.3e}")
    if near:
        assert b["margin"] > 1e-4, b["margin"]                      # nothing near a threshold: fp32, fp64 and the device must agree
    if populated and P >= 63:
        for k in ("kept", "clones", "split", "pruned"):
            assert b[k] >= math.ceil(0.05 * P), (k, b[k])
    out = bag.densify_and_prune(opt, noise=z.to(DEV), N=N, screen_size=mode, **rule)
    for k in ("kept", "clones", "split", "pruned", "P_new"):
        assert out[k] == a[k] == b[k], (k, out[k], a[k], b[k])
    assert out["provenance"].dtype == torch.int32 and torch.equal(out["provenance"].cpu().long(), b["provenance"])
    assert torch.equal(a["provenance"], b["provenance"])
    kind = b["provenance"][:, 1]
    p, p32, p64 = D.params(opt), D.params(ref32), D.params(ref64)
    for n in R.NAMES:
        q = p[n]
        assert q is getattr(bag, LEAF[n]) and q.is_leaf and q.requires_grad and q.grad is None and q.is_cuda, n
        assert q.shape == p32[n].shape, (n, q.shape, p32[n].shape)
        got = q.detach().cpu()
        if n in ("xyz", "scaling"):
            old = kind < D.CHILD
            assert torch.equal(got[old], p32[n].detach()[old]), n
            if int((~old).sum()):
                R.assert_rule(f"{label}/children.{n}", got[~old], p32[n].detach()[~old], p64[n].detach()[~old])
        else:
            assert torch.equal(got, p32[n].detach()), n
        st, st32 = _state(opt, q), _state(ref32, p32[n])
        assert (st is None) == (st32 is None) == (steps[n] is None), n
        if st is not None:
            assert float(st["step"]) == steps[n] == float(st32["step"]) and not st["step"].is_cuda, n
            for key in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(st[key].cpu(), st32[key]), (n, key)              # kept rows bit for bit, new rows exact zeros
                if int((kind != D.KEPT).sum()) and st[key].numel():                 # (a group of width 0 has no element to look at)
                    assert st[key].cpu()[kind != D.KEPT].abs().max().item() == 0.0
    assert len(opt.state) == sum(s is not None for s in steps.values())           # the old parameters' entries are gone
    for name, shape in (("xyz_gradient_accum", (b["P_new"], 1)), ("denom", (b["P_new"], 1)), ("max_radii2D", (b["P_new"],))):
        t = getattr(bag, name)
        assert tuple(t.shape) == shape and t.is_cuda and (t.numel() == 0 or t.abs().max().item() == 0.0), name
    return out, b


@pytest.mark.parametrize("P", [1, 63, 1001, 100_003])
def test_equals_the_restatement(P):
    opt, bag, stats, noise = _case(P, seed=P)
    _compare(f"P={P}", opt, bag, stats, noise)


@pytest.mark.timeout(900)
def test_equals_the_restatement_at_bench_size():
    opt, bag, stats, noise = _case(500_000, seed=500_000)
    _compare("P=500000", opt, bag, stats, noise)


def test_three_children_and_the_pre_densify_switch():
    opt, bag, stats, noise = _case(1001, seed=1001)
    _compare("N=3", opt, bag, stats, noise, N=3)
    opt, bag, stats, noise = _case(100_003, seed=100_003)
    pub = D.densify_and_prune(D.clone_optimizer(opt), {k: v.cpu() for k, v in stats.items()}, noise=noise[:, :2], **D.RULE)
    out, ref = _compare("pre_densify", opt, bag, stats, noise, mode="pre_densify")
    assert ref["pruned"] > pub["pruned"] and ref["kept"] < pub["kept"]            # the switch does something on these inputs


def test_plumbing_step_render_and_state_dict():
    """After the call the bag's leaves are the optimizer's parameters; a GaussianAdam step and a rasterizer forward + backward run
    on the new set, and state_dict() round-trips."""
    from bags_raster import GaussianAdam
    from bags_raster.render import render, PipelineParams
    from bags_raster.synth import sphere_views
    opt, bag, stats, noise = _case(1001, seed=4)
    with torch.no_grad():
        bag._xyz.mul_(0.2)                                         # in front of the camera
    out, _ = _compare("plumbing", opt, bag, stats, noise)
    assert [g["params"][0] for g in opt.param_groups] == [getattr(bag, LEAF[n]) for n in R.NAMES]
    cam = sphere_views(1, 96, 64, device=DEV)[0]
    res = render(cam, bag, PipelineParams(), torch.zeros(3, device=DEV), 0.0, None, hybrid=False)
    res["render"].sum().backward()
    assert all(t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad).all() for t in bag.leaves())
    assert res["radii"].numel() == out["P_new"] and int((res["radii"] > 0).sum()) > 0
    before = bag._features_dc.detach().clone()
    opt.step(stats=(bag, res["viewspace_points"], res["radii"]))
    assert not torch.equal(before, bag._features_dc.detach()) and bag.denom.sum().item() > 0
    assert all(float(opt.state[q]["step"]) == 4.0 and opt.state[q]["exp_avg"].shape == q.shape for q in bag.leaves())
    sd = opt.state_dict()
    twin = GaussianAdam(R.param_groups([torch.nn.Parameter(torch.zeros_like(g["params"][0])) for g in opt.param_groups]), lr=0.0, eps=R.EPS)
    twin.load_state_dict(sd)
    sd2 = twin.state_dict()
    assert sd["param_groups"] == sd2["param_groups"] and sd["state"].keys() == sd2["state"].keys()
    for k in sd["state"]:
        for name in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sd["state"][k][name].cpu(), sd2["state"][k][name].cpu()), (k, name)


def test_nothing_selected_and_everything_pruned():
    opt, bag, stats, noise = _case(1001, seed=7)
    before = [(q.detach().clone(), opt.state[q]["exp_avg"].clone(), opt.state[q]["exp_avg_sq"].clone()) for q in bag.leaves()]
    idle = dict(D.RULE, max_grad=1e9, min_opacity=0.0, max_screen_size=None)
    out, _ = _compare("nothing", opt, bag, stats, noise, rule=idle, populated=False, near=False)
    assert (out["kept"], out["clones"], out["split"], out["pruned"], out["P_new"]) == (1001, 0, 0, 0, 1001)
    assert torch.equal(out["provenance"].cpu(), torch.stack((torch.arange(1001), torch.zeros(1001, dtype=torch.long)), 1).int())
    for q, (p0, m0, v0) in zip(bag.leaves(), before):               # the set unchanged bit for bit, the statistics still zeroed
        assert torch.equal(q.detach(), p0) and torch.equal(opt.state[q]["exp_avg"], m0) and torch.equal(opt.state[q]["exp_avg_sq"], v0)
    gone = dict(D.RULE, min_opacity=1.5)
    out, _ = _compare("everything", opt, bag, {k: getattr(bag, k) for k in stats}, noise, rule=gone, populated=False, near=False)
    assert out["P_new"] == 0 and out["kept"] == 0 and all(q.shape[0] == 0 for q in bag.leaves())
    again = bag.densify_and_prune(opt, **D.RULE)                    # the empty set: a no-op
    assert again["P_new"] == 0 and again["pruned"] == 0


def test_without_state_and_with_torch_adam():
    opt, bag, stats, noise = _case(1001, seed=8, steps=0)
    opt.state.clear()                                               # no step taken: no state, and none afterwards
    _compare("stateless", opt, bag, stats, noise)
    assert len(opt.state) == 0
    opt, bag, stats, noise = _case(1001, seed=9, opt_cls=torch.optim.Adam)
    _compare("torch.optim.Adam", opt, bag, stats, noise)
    for q, gr in zip(bag.leaves(), range(6)):
        q.grad = torch.full_like(q, 0.01)
    opt.step()                                                      # torch.optim.Adam goes on with the moved state
    assert all(float(opt.state[q]["step"]) == 4.0 for q in bag.leaves())


def test_degree_zero_bag():
    """SH degree 0: ``_features_rest`` is (P,0,3), a group with nothing to move.  It is left out of the launch (as relocate and add_new
    leave it out) and comes back (P_new,0,3), installed in the optimizer like the other five; before csrc/row_rebuild.h the call raised
    ``group 2: width 0 <= 0``.  The restatement on the CPU, fp32 and fp64: kept 11, clones 11, split 54, pruned 0, P_new 130, margin
    6.8e-3; nothing is pruned, hence populated=False."""
    import mcmc_reference as M
    from bags_raster import GaussianAdam
    opt, stats = M.make_case(65, 1, GaussianAdam, DEV, sh_degree=0)
    bag = _bag_of(opt, stats, GaussianBag(0))
    bag.active_sh_degree = 0
    noise = torch.randn(65, 2, 3, generator=torch.Generator().manual_seed(65))
    out, ref = _compare("degree0", opt, bag, stats, noise, populated=False)
    assert (ref["kept"], ref["clones"], ref["split"], ref["pruned"], ref["P_new"]) == (11, 11, 54, 0, 130)
    rest = bag._features_rest
    assert tuple(rest.shape) == (130, 0, 3) and rest is D.params(opt)["f_rest"] and rest.is_leaf and rest.requires_grad
    assert len(opt.state) == 6 and tuple(opt.state[rest]["exp_avg"].shape) == tuple(opt.state[rest]["exp_avg_sq"].shape) == (130, 0, 3)


def _run(seed_case, **kw):
    opt, bag, stats, noise = _case(20_011, seed=seed_case)
    out = bag.densify_and_prune(opt, **dict(D.RULE, **kw))
    return out, [q.detach().clone() for q in bag.leaves()], [opt.state[q]["exp_avg_sq"].clone() for q in bag.leaves()]


def test_two_calls_are_bitwise_equal_and_the_seed_decides_the_children():
    opt, bag, stats, noise = _case(20_011, seed=11)
    z = noise[:, :2].contiguous().to(DEV)
    a = bag.densify_and_prune(opt, noise=z, **D.RULE)
    first = [q.detach().clone() for q in bag.leaves()] + [opt.state[q]["exp_avg"].clone() for q in bag.leaves()]
    opt, bag, stats, noise = _case(20_011, seed=11)
    b = bag.densify_and_prune(opt, noise=z, **D.RULE)
    assert torch.equal(a["provenance"], b["provenance"])
    assert all(torch.equal(x, y) for x, y in zip(first, [q.detach().clone() for q in bag.leaves()] + [opt.state[q]["exp_avg"] for q in bag.leaves()]))
    # the generator inside the kernel
    r1, p1, v1 = _run(11, seed=1234)
    r2, p2, v2 = _run(11, seed=1234)
    r3, p3, v3 = _run(11, seed=1235)
    assert torch.equal(r1["provenance"], r2["provenance"]) and torch.equal(r1["provenance"], r3["provenance"])
    assert all(torch.equal(x, y) for x, y in zip(p1 + v1, p2 + v2))                 # same seed: identical bits
    child = r1["provenance"][:, 1] >= D.CHILD
    assert int(child.sum()) > 1000
    assert not (p1[0][child] == p3[0][child]).all(dim=1).any()                     # another seed: every child moved
    assert all(torch.equal(x[~child], y[~child]) for x, y in zip(p1, p3)) and all(torch.equal(x, y) for x, y in zip(p1[1:4] + p1[5:], p3[1:4] + p3[5:]))
    torch.manual_seed(77)
    r4, p4, _ = _run(11)
    torch.manual_seed(77)
    r5, p5, _ = _run(11)
    assert torch.equal(p4[0], p5[0]) and not torch.equal(p4[0], p1[0])              # seed=None: torch's CPU generator governs


def test_in_kernel_generator_is_standard_normal():
    """z = R^T (xyz_child - xyz_parent) / exp(scaling) recovered for n >= 1e5 values: |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n)
    (five standard errors of the mean and of the variance of n standard normals), and no two children of one parent equal."""
    opt, bag, stats, noise = _case(100_003, seed=100_003)
    xyz0, sc0, rot0 = bag._xyz.detach().double().cpu(), bag._scaling.detach().double().cpu(), bag._rotation.detach().double().cpu()
    out = bag.densify_and_prune(opt, seed=2024, **D.RULE)
    prov = out["provenance"].cpu().long()
    child = prov[:, 1] >= D.CHILD
    src = prov[child, 0]
    Rm = D.build_rotation(rot0[src])
    d = bag._xyz.detach().double().cpu()[child] - xyz0[src]
    z = torch.bmm(Rm.transpose(1, 2), d.unsqueeze(-1)).squeeze(-1) / torch.exp(sc0[src])
    n = z.numel()
    mean, var = z.mean().item(), z.var().item()
    print(f"DENSIFY generator: n {n} mean {mean:.3e} (bound {5 / math.sqrt(n):.3e}) var - 1 {var - 1:.3e} (bound {5 * math.sqrt(2 / n):.3e}) "
          f"max |z| {z.abs().max().item():.3f}")
    assert n >= 100_000
    assert abs(mean) <= 5 / math.sqrt(n) and abs(var - 1) <= 5 * math.sqrt(2 / n)
    for axis in range(3):
        assert abs(z[:, axis].mean().item()) <= 5 / math.sqrt(n / 3) and abs(z[:, axis].var().item() - 1) <= 5 * math.sqrt(6 / n)
    S = int(child.sum()) // 2
    first, second = bag._xyz.detach()[child.to(DEV)][:S], bag._xyz.detach()[child.to(DEV)][S:]
    assert torch.equal(prov[child][:S, 0], prov[child][S:, 0]) and not (first == second).all(dim=1).any()


@pytest.mark.parametrize("P", [1, 63, 100_003])
def test_reset_opacity(P):
    opt, bag, stats, noise = _case(P, seed=P + 1)
    ref32, ref64 = D.clone_optimizer(opt), D.clone_optimizer(opt, dtype=torch.float64)
    others = [(q.detach().clone(), opt.state[q]["exp_avg"].clone()) for q in bag.leaves() if q is not bag._opacity]
    bag._opacity.grad = torch.ones_like(bag._opacity)
    bag.reset_opacity(opt)
    a, b = D.reset_opacity(ref32), D.reset_opacity(ref64)
    R.assert_rule(f"reset_opacity/P={P}", bag._opacity.detach(), a.detach(), b.detach())
    assert torch.sigmoid(bag._opacity.detach()).max().item() <= 0.01 * (1 + 1e-6)
    st = opt.state[bag._opacity]
    assert st["exp_avg"].abs().max().item() == 0.0 and st["exp_avg_sq"].abs().max().item() == 0.0 and float(st["step"]) == 3.0
    assert D.params(opt)["opacity"] is bag._opacity and bag._opacity.grad is None and bag._opacity.requires_grad
    for (p0, m0), q in zip(others, [q for q in bag.leaves() if q is not bag._opacity]):
        assert torch.equal(q.detach(), p0) and torch.equal(opt.state[q]["exp_avg"], m0)
    fresh, bag2, _, _ = _case(63, seed=3, steps=0)
    fresh.state.clear()
    bag2.reset_opacity(fresh)                                      # no state: the parameter alone
    assert len(fresh.state) == 0 and torch.sigmoid(bag2._opacity.detach()).max().item() <= 0.01 * (1 + 1e-6)


def _gap_threshold(values, lo, hi, extra=None):
    """A threshold for ``values`` between their ``lo`` and ``hi`` quantiles, in the middle of the widest relative gap between two
    neighbours there.  Returns (threshold, margin): margin = half the gap over the threshold, or less where ``extra(threshold)``
    (the margin of something else that hangs on the same threshold) is smaller."""
    v = values.detach().double().reshape(-1).sort().values.cpu()
    n = v.numel()
    best = (-1.0, None)
    for i in range(max(int(lo * n), 1), min(max(int(hi * n), int(lo * n) + 2), n)):
        t = float(v[i - 1] + v[i]) / 2
        m = float(v[i] - v[i - 1]) / 2 / t if t > 0 else 0.0
        if extra is not None and m > best[0]:
            m = min(m, extra(t))
        if m > best[0]:
            best = (m, t)
    return best[1], best[0]


@pytest.mark.timeout(900)
def test_end_to_end_three_rounds():
    """Three rounds of {10 iterations, densify-and-prune, opacity reset} on a synthetic scene, three times from one start:
    A  GaussianAdam (statistics folded into the step) + the fused calls;
    B  torch.optim.Adam + add_densification_stats + the restatement, fp32, on the GPU;
    C  as B with float64 parameters, moments and restatement (the rasterizer is fed their fp32 rounding).
    All three use the same noise and the same thresholds.  The thresholds of a round are taken by run A from its own statistics,
    each in the middle of the widest gap of the data near the quantile it aims at (max_grad near the median, percent_dense * extent in the
    middle half, min_opacity in the lowest 5 %; 0.1 * extent, which hangs on extent, is counted in; the margins
    are printed); every run, A included, then asserts on its own state that no tested value lies within 1e-4 relative of a threshold.  So the
    three runs, whose states differ by rounding and its growth over ten iterations, must take the same decisions: P agrees among
    all three after every round.  At every densification of A the restatement is also run on a copy of A's own state: order and
    copied quantities equal, children within the rule (_compare).  The loss: B and C differ by nothing but the precision of the
    PyTorch route, so |loss_B - loss_C| after the last iteration is the spread that route shows against itself, and the final loss
    of A must lie within it of C."""
    from bags_raster import GaussianAdam
    from bags_raster.loss import fused_photometric_loss
    from bags_raster.render import render, PipelineParams
    from bags_raster.synth import synth_scene, sphere_views
    P0, W, H = 3000, 160, 112
    scene = synth_scene(P0, 0, 0.5, 3)
    cam = sphere_views(1, W, H, device=DEV)[0]
    target = dict(scene)
    target["shs"] = scene["shs"].clone()
    target["shs"][:, 0, :] += 0.5
    bg, pipe = torch.zeros(3, device=DEV), PipelineParams()
    with torch.no_grad():
        gt = render(cam, GaussianBag.from_activated(target, 3, device=DEV), pipe, bg, 0.0, None, hybrid=False)["render"].clone()
    gen = torch.Generator().manual_seed(21)
    noises, rules = {}, {}

    def thresholds(bag, stats):
        g = (stats["xyz_gradient_accum"] / stats["denom"]).nan_to_num(0.0).reshape(-1)
        s = torch.exp(bag._scaling.detach()).max(dim=1).values.double()
        tested = torch.cat((s, s / 1.6))                              # 0.1 * extent is compared with rows and with children (N = 2)
        max_grad, m_g = _gap_threshold(g[g > 0], 0.4, 0.6)
        thr, m_s = _gap_threshold(s, 0.25, 0.75, extra=lambda t: float(((tested - 10 * t).abs() / (10 * t)).min()))
        min_opacity, m_o = _gap_threshold(torch.sigmoid(bag._opacity.detach()), 0.005, 0.05)
        print(f"DENSIFY end_to_end thresholds: max_grad {max_grad:.6e} (margin {m_g:.2e}) thr {thr:.6e} ({m_s:.2e}) min_opacity {min_opacity:.6e} ({m_o:.2e})")
        return dict(max_grad=max_grad, min_opacity=min_opacity, extent=thr / 0.01, max_screen_size=20, percent_dense=0.01)

    def run(kind):
        bag = GaussianBag.from_activated(scene, 3, device=DEV)              # the fp32 set that is rendered
        groups = R.param_groups([bag._xyz, bag._features_dc, bag._features_rest, bag._opacity, bag._scaling, bag._rotation])
        if kind == "A":
            opt = GaussianAdam(groups, lr=0.0, eps=R.EPS)
        elif kind == "B":
            opt = torch.optim.Adam(groups, lr=0.0, eps=R.EPS)
        else:
            master = [torch.nn.Parameter(g["params"][0].detach().double()) for g in groups]
            opt = torch.optim.Adam(R.param_groups(master), lr=0.0, eps=R.EPS)
        losses, sizes = [], []
        for rnd in range(3):
            for it in range(10):
                for t in bag.leaves():
                    t.grad = None
                out = render(cam, bag, pipe, bg, 0.0, None, hybrid=False)
                loss = fused_photometric_loss(out["render"], gt)
                loss.backward()
                losses.append(loss.item())
                if kind == "A":
                    opt.step(stats=(bag, out["viewspace_points"], out["radii"]))
                    continue
                vis = out["radii"] > 0
                bag.add_densification_stats(out["viewspace_points"], out["viewspace_points_densify"], vis, False)
                bag.max_radii2D[vis] = torch.max(bag.max_radii2D[vis], out["radii"][vis].float())
                if kind == "C":
                    for n, q in D.params(opt).items():
                        q.grad = getattr(bag, LEAF[n]).grad.double()
                opt.step()
                if kind == "C":
                    for n, q in D.params(opt).items():
                        setattr(bag, LEAF[n], q.detach().float().requires_grad_(True))
            P = bag._xyz.shape[0]
            stats = {k: getattr(bag, k) for k in ("xyz_gradient_accum", "denom", "max_radii2D")}
            if kind == "A":
                noises[rnd] = torch.randn(P, 2, 3, generator=gen)
                rules[rnd] = thresholds(bag, stats)
            z, rule = noises[rnd], rules[rnd]
            assert z.shape[0] == P, (kind, rnd, P, z.shape[0])
            if kind == "A":
                _compare(f"end_to_end/round{rnd}", opt, bag, stats, z, rule=rule, populated=False, near=True)
                bag.reset_opacity(opt)
            else:
                res = D.densify_and_prune(opt, stats, noise=z.to(DEV), **rule)
                print(f"DENSIFY end_to_end/round{rnd} run {kind}: P {P} -> {res['P_new']} margin {res['margin']:.3e}")
                assert res["margin"] > 1e-4, (kind, rnd, res["margin"])
                D.reset_opacity(opt)
                _bag_of(opt, {k: v.float() for k, v in res["stats"].items()}, bag)
                if kind == "C":
                    for n, q in D.params(opt).items():
                        setattr(bag, LEAF[n], q.detach().float().requires_grad_(True))
            sizes.append(bag._xyz.shape[0])
        return losses, sizes
    (la, sa), (lb, sb), (lc, sc) = run("A"), run("B"), run("C")
    print("DENSIFY end_to_end sizes", sa, sb, sc)
    assert sa == sb == sc and sa[0] != P0
    spread, ours = abs(lb[-1] - lc[-1]), abs(la[-1] - lc[-1])
    print(f"DENSIFY end_to_end loss: first {la[0]:.6f} last A {la[-1]:.9f} B {lb[-1]:.9f} C {lc[-1]:.9f}; |A - C| {ours:.3e}, spread |B - C| {spread:.3e}; "
          f"over the 30 iterations max |A - B| {max(abs(x - y) for x, y in zip(la, lb)):.3e}")
    assert ours <= spread
