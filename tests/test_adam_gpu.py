"""GaussianAdam on the MI355X against torch.optim.Adam.  Every numerical check follows tests/adam_reference.py: the reference is
torch.optim.Adam in float64 on the CPU from the same fp32 state and gradients, and the bound is PyTorch's own fp32 error
against it, err(kernel) <= 2 * err(torch fp32) + 1, measured in the same test.

Largest (err(kernel), err(torch fp32)) pairs measured on an MI355X are recorded in profiles/adam/NOTES.md."""
import pytest
import torch

import adam_reference as R
from bags_raster.optim import GaussianAdam  # noqa: F401  (the feature under test: without it nothing here can pass)

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ours(states, step=0, **kw):
    from bags_raster import GaussianAdam
    return R.build(GaussianAdam, states, DEV, torch.float32, step, **kw)


def _check_against(label, ours, torch32, ref64):
    """ours / torch32 / ref64: snapshot() lists; parameters and both moments under the rule, step counts equal."""
    for i, (a, b, r) in enumerate(zip(ours, torch32, ref64)):
        assert a[3] == b[3] == r[3], (label, i, a[3], b[3], r[3])
        for name, x, y, z in zip(R.KEYS, a, b, r):
            R.assert_rule(f"{label}/{R.NAMES[i % 6]}.{name}", x, y, z)


@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("P", [1, 63, 1001, 100_003])
def test_one_step_all_six_widths(P, step):
    states = R.random_state(P, seed=1000 * step + P % 997)
    opt, params = _ours(states, step - 1)
    opt.step()
    _check_against(f"one_step[P={P},step={step}]", R.snapshot(opt, params), R.torch_adam_step(states, step, torch.float32),
                   R.torch_adam_step(states, step, torch.float64))


class Trio:
    """The same optimisation driven three ways: GaussianAdam (GPU), torch.optim.Adam fp32 (GPU), torch.optim.Adam fp64 (CPU)."""

    def __init__(self, states, torch32_kw=None):
        self.runs = [_ours(states), R.build(torch.optim.Adam, states, DEV, torch.float32, **(torch32_kw or {})),
                     R.build(torch.optim.Adam, states, "cpu", torch.float64)]
        self.runs = [[o, p] for o, p in self.runs]

    def step(self, grads, lr0=None):
        for opt, params in self.runs:
            if lr0 is not None:
                opt.param_groups[0]["lr"] = lr0                     # update_learning_rate: a write to the xyz group's lr
            for p, g in zip(params, grads):
                p.grad = None if g is None else g.to(p.device, p.dtype)
            opt.step()

    def surgery(self, fn, *args):
        for run in self.runs:
            run[1] = fn(run[0], *args)

    def check(self, label):
        _check_against(label, *[R.snapshot(o, p) for o, p in self.runs])


def _grads(P, seed, shapes=R.SHAPES):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((P,) + s, generator=g) * 0.01 * (torch.rand(P, generator=g) < 0.8).reshape((P,) + (1,) * len(s)) for s in shapes]


def test_fifty_steps_with_a_changing_learning_rate():
    P = 5003
    trio = Trio(R.random_state(P, seed=5))
    for it in range(50):
        trio.step(_grads(P, 100 + it), lr0=0.00016 * (0.01 ** (it / 50.0)))
    trio.check("fifty_steps")
    assert trio.runs[0][0].state[trio.runs[0][1][0]]["step"].item() == 50.0


def test_group_without_grad_and_all_zero_grads():
    P = 777
    states = R.random_state(P, seed=11)
    states[2]["grad"] = None
    states[4]["grad"] = torch.zeros_like(states[4]["grad"])
    opt, params = _ours(states, step=4)
    opt.step()
    got = R.snapshot(opt, params)
    for name, x in zip(R.KEYS, got[2]):
        assert torch.equal(x.cpu(), states[2][name]), name            # untouched ...
    assert got[2][3] == 4.0 and got[0][3] == 5.0                       # ... and its step does not advance
    # all-zero gradients still move the parameters by momentum in dense mode, as in PyTorch
    assert not torch.equal(got[4][0].cpu(), states[4]["param"])
    _check_against("zero_grad", got, R.torch_adam_step(states, 5, torch.float32), R.torch_adam_step(states, 5, torch.float64))


@pytest.mark.parametrize("P", [5, 1001, 50_001])
def test_visible_only_is_the_dense_step_on_visible_rows(P):
    states = R.random_state(P, seed=P)
    vis = torch.rand(P, generator=torch.Generator().manual_seed(2)) < 0.3
    radii = torch.where(vis, torch.randint(1, 40, (P,), generator=torch.Generator().manual_seed(3)),
                        torch.randint(-2, 1, (P,), generator=torch.Generator().manual_seed(4))).to(torch.int32)
    dense_opt, dense_p = _ours(states, step=7)
    dense_opt.step()
    dense = R.snapshot(dense_opt, dense_p)
    for mask in (radii.to(DEV), vis.to(DEV)):                          # int32 (zero and negative entries are not visible) and bool
        opt, params = _ours(states, step=7)
        opt.step(visibility=mask)
        got = R.snapshot(opt, params)
        for i, (a, d, s) in enumerate(zip(got, dense, states)):
            assert a[3] == 8.0                                         # bias corrections follow the group's global step count
            for name, x, y in zip(R.KEYS, a, d):
                x, y = x.cpu(), y.cpu()
                assert torch.equal(x[~vis], s[name][~vis]), (i, name, "a hidden row changed")
                assert torch.equal(x[vis], y[vis]), (i, name, "a visible row differs from the dense step")
    _check_against(f"visible[P={P}]", got, R.torch_adam_step(states, 8, torch.float32, visible=vis),
                   R.torch_adam_step(states, 8, torch.float64, visible=vis))
    with pytest.raises(RuntimeError, match="visibility has"):
        opt.step(visibility=torch.ones(P + 1, dtype=torch.int32, device=DEV))
    with pytest.raises(TypeError, match="visibility must be int32"):
        opt.step(visibility=torch.ones(P, dtype=torch.float32, device=DEV))


def test_unaligned_groups_take_the_scalar_path():
    """Parameters, gradients and moments that start 4 bytes into an allocation: no float4 access, same bits as the aligned step."""
    from bags_raster import GaussianAdam
    P = 4099
    states = R.random_state(P, seed=21)
    ref_opt, ref_p = _ours(states, step=2)
    ref_opt.step()
    want = R.snapshot(ref_opt, ref_p)

    def shifted(t):
        buf = torch.empty(t.numel() + 1, device=DEV)
        view = buf[1:].view(t.shape)
        view.copy_(t)
        assert view.data_ptr() % 16 == 4
        return view
    vis = (torch.rand(P, generator=torch.Generator().manual_seed(1)) < 0.5).to(DEV)
    for mask in (None, vis):
        params = [shifted(s["param"]).requires_grad_(True) for s in states]
        opt = GaussianAdam(R.param_groups(params), lr=0.0, betas=R.BETAS, eps=R.EPS)
        for p, s in zip(params, states):
            opt.state[p] = {"step": torch.tensor(2.0), "exp_avg": shifted(s["exp_avg"]), "exp_avg_sq": shifted(s["exp_avg_sq"])}
            p.grad = shifted(s["grad"])
        opt.step(visibility=mask)
        for i, (p, w, s) in enumerate(zip(params, want, states)):
            for name, x, y in zip(R.KEYS, (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]), w):
                if mask is None:
                    assert torch.equal(x, y), (i, name)
                else:
                    assert torch.equal(x[mask], y[mask]) and torch.equal(x[~mask].cpu(), s[name][~mask.cpu()]), (i, name)


def test_input_errors_on_the_gpu():
    from bags_raster import GaussianAdam
    p = torch.nn.Parameter(torch.zeros(8, 3, device=DEV))
    opt = GaussianAdam([{"params": [p], "lr": 1e-3, "name": "xyz"}], lr=0.0, eps=1e-15)
    p.grad = torch.ones(3, 8, device=DEV).t()
    with pytest.raises(RuntimeError, match="contiguous"):
        opt.step()
    q = torch.nn.Parameter(torch.zeros(8, 3, device=DEV, dtype=torch.float64))
    q.grad = torch.ones_like(q)
    with pytest.raises(TypeError, match="float32"):
        GaussianAdam([q]).step()
    assert len(opt.state) == 0                                         # refused before any state was made or counted


def _scene_backward(P=3000, W=160, H=112, seed=0):
    from bags_raster.gaussians import GaussianBag
    from bags_raster.loss import fused_photometric_loss
    from bags_raster.render import render, PipelineParams
    from bags_raster.synth import synth_scene, sphere_views
    scene = synth_scene(P, seed, 0.5, 3)
    cam = sphere_views(1, W, H, device=DEV)[0]
    target = dict(scene)
    target["shs"] = scene["shs"].clone()
    target["shs"][:, 0, :] += 0.5
    bg = torch.zeros(3, device=DEV)
    pipe = PipelineParams()
    with torch.no_grad():
        gt = render(cam, GaussianBag.from_activated(target, 3, device=DEV), pipe, bg, 0.0, None, hybrid=False)["render"].clone()

    def iteration(bag):
        for t in bag.leaves():
            t.grad = None
        out = render(cam, bag, pipe, bg, 0.0, None, hybrid=False)
        loss = fused_photometric_loss(out["render"], gt)
        loss.backward()
        return loss.item(), out
    return scene, iteration


def _bag_groups(bag):
    # training_setup's order and names (scene/gaussian_model.py:192-210)
    return R.param_groups([bag._xyz, bag._features_dc, bag._features_rest, bag._opacity, bag._scaling, bag._rotation])


@pytest.mark.parametrize("abs_grad", [False, True])
def test_stats_block_equals_add_densification_stats(abs_grad):
    from bags_raster import GaussianAdam
    from bags_raster.gaussians import GaussianBag
    scene, iteration = _scene_backward()
    bag = GaussianBag.from_activated(scene, 3, device=DEV)
    _, out = iteration(bag)
    radii = out["radii"]
    assert radii.dtype == torch.int32 and 0 < int((radii > 0).sum()) < radii.numel()
    P = radii.numel()
    g = torch.Generator().manual_seed(8)
    start = dict(xyz_gradient_accum=torch.rand(P, 1, generator=g).to(DEV), denom=torch.randint(0, 9, (P, 1), generator=g).float().to(DEV),
                 max_radii2D=(torch.rand(P, generator=g) * 30).to(DEV))
    vis = radii > 0
    view = out["viewspace_points_densify" if abs_grad else "viewspace_points"]
    # PyTorch: the four indexed ops of an iteration
    want = GaussianBag(3)
    for k, v in start.items():
        setattr(want, k, v.clone())
    want.add_densification_stats(out["viewspace_points"], out["viewspace_points_densify"], vis, abs_grad)
    want.max_radii2D[vis] = torch.max(want.max_radii2D[vis], radii[vis])
    # float64 evaluation of the same update
    acc64 = start["xyz_gradient_accum"].double().cpu()
    acc64[vis.cpu()] += torch.norm(view.grad.double().cpu()[vis.cpu(), :2], dim=-1, keepdim=True)
    for k, v in start.items():
        setattr(bag, k, v.clone())
    opt = GaussianAdam(_bag_groups(bag), lr=0.0, eps=1e-15)
    opt.step(stats=(bag, view, radii))
    assert torch.equal(bag.denom, want.denom) and torch.equal(bag.max_radii2D, want.max_radii2D)
    R.assert_rule(f"stats[abs_grad={abs_grad}]/xyz_gradient_accum", bag.xyz_gradient_accum, want.xyz_gradient_accum, acc64)
    for k, v in start.items():
        assert torch.equal(getattr(bag, k)[~vis], v[~vis]), k            # rows with radii == 0: bitwise unchanged
    assert not torch.equal(bag.xyz_gradient_accum[vis], start["xyz_gradient_accum"][vis])
    # radii from a real forward is accepted as the visibility mask, together with the statistics
    before = [t.detach().clone() for t in bag.leaves()]
    opt.step(visibility=radii, stats=(bag, view, radii))
    assert torch.equal(bag.denom[vis], want.denom[vis] + 1)
    for t, b in zip(bag.leaves(), before):
        assert torch.equal(t[~vis], b[~vis])
    assert not torch.equal(bag._opacity[vis], before[5][vis])
    with pytest.raises(RuntimeError, match="screen-space gradient must be"):
        opt.step(stats=(bag, view, radii[:-1].contiguous()))


def test_two_runs_are_bitwise_equal():
    P = 20_011
    states = R.random_state(P, seed=31)
    vis = (torch.rand(P, generator=torch.Generator().manual_seed(5)) < 0.5).to(DEV)
    for mask in (None, vis):
        runs = []
        for _ in range(2):
            opt, params = _ours(states, step=3)
            for it in range(3):
                opt.step(visibility=mask)
            runs.append(R.snapshot(opt, params))
        for a, b in zip(*runs):
            assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))


def test_densification_surgery():
    P = 2001
    trio = Trio(R.random_state(P, seed=41))
    for it in range(3):
        trio.step(_grads(P, 200 + it))
    g = torch.Generator().manual_seed(42)
    trio.surgery(R.cat_tensors_to_optimizer, [torch.randn((500,) + s, generator=g) for s in R.SHAPES])
    P += 500
    for it in range(3):
        trio.step(_grads(P, 300 + it))
    trio.check("surgery_cat")
    trio.surgery(R.prune_optimizer, torch.rand(P, generator=g) < 0.7)
    P = trio.runs[0][1][0].shape[0]
    assert 0 < P < 2501 and trio.runs[2][1][0].shape[0] == P
    for it in range(3):
        trio.step(_grads(P, 400 + it))
    trio.check("surgery_prune")
    assert trio.runs[0][0].state[trio.runs[0][1][2]]["step"].item() == 9.0


def test_state_interchange_with_torch_adam():
    from bags_raster import GaussianAdam
    P, k = 1501, 5
    states = R.random_state(P, seed=51)
    trio = Trio(states)
    first, first_p = R.build(torch.optim.Adam, states, DEV, torch.float32)
    for it in range(k):
        gr = _grads(P, 500 + it)
        for p, g in zip(first_p, gr):
            p.grad = g.to(DEV)
        first.step()
        for run in trio.runs[1:]:
            for p, g in zip(run[1], gr):
                p.grad = g.to(p.device, p.dtype)
            run[0].step()
    # hand over: the parameters as they are, the state through state_dict()
    params = [torch.nn.Parameter(p.detach().clone()) for p in first_p]
    ours = GaussianAdam(R.param_groups(params), lr=0.0, betas=R.BETAS, eps=R.EPS)
    ours.load_state_dict(first.state_dict())
    trio.runs[0] = [ours, params]
    for it in range(k):
        trio.step(_grads(P, 600 + it))
    trio.check("interchange")
    assert ours.state[params[0]]["step"].item() == 2.0 * k
    # and back into torch.optim.Adam
    back, back_p = R.build(torch.optim.Adam, states, DEV, torch.float32)
    back.load_state_dict(ours.state_dict())
    assert torch.equal(back.state[back_p[2]]["exp_avg"], ours.state[params[2]]["exp_avg"])


def test_end_to_end_training_iterations():
    """30 iterations of render -> fused loss -> backward -> step on a small synthetic scene, once with
    GaussianAdam.step(radii, stats) and once with torch.optim.Adam + add_densification_stats, from the same start.  The loss
    falls in both.  Each run is shadowed by a float64 torch.optim.Adam on the CPU that is fed the run's own fp32 gradients, so
    the rasterizer's round-off is not counted: err(GaussianAdam run against its shadow) obeys the rule with err(PyTorch run
    against its shadow) as the yardstick."""
    from bags_raster import GaussianAdam
    from bags_raster.gaussians import GaussianBag
    scene, iteration = _scene_backward()
    results = {}
    for kind in ("ours", "torch"):
        bag = GaussianBag.from_activated(scene, 3, device=DEV)
        opt = (GaussianAdam if kind == "ours" else torch.optim.Adam)(_bag_groups(bag), lr=0.0, eps=1e-15)
        shadow_p = [torch.nn.Parameter(g["params"][0].detach().double().cpu()) for g in opt.param_groups]
        shadow = torch.optim.Adam(R.param_groups(shadow_p), lr=0.0, eps=1e-15)
        losses = []
        for it in range(30):
            loss, out = iteration(bag)
            losses.append(loss)
            for sp, grp in zip(shadow_p, opt.param_groups):
                sp.grad = grp["params"][0].grad.double().cpu()
            shadow.step()
            if kind == "ours":
                opt.step(stats=(bag, out["viewspace_points"], out["radii"]))        # dense, as the reference steps
            else:
                vis = out["radii"] > 0
                bag.add_densification_stats(out["viewspace_points"], out["viewspace_points_densify"], vis, False)
                bag.max_radii2D[vis] = torch.max(bag.max_radii2D[vis], out["radii"][vis])
                opt.step()
        assert losses[-1] < losses[0], (kind, losses[0], losses[-1])
        results[kind] = ([g["params"][0].detach().clone() for g in opt.param_groups], [p.detach().clone() for p in shadow_p], bag, losses)
    print("ADAM_E2E losses", {k: (v[3][0], v[3][-1]) for k, v in results.items()})
    for i, name in enumerate(R.NAMES):
        ek, et = R.err(results["ours"][0][i], results["ours"][1][i]), R.err(results["torch"][0][i], results["torch"][1][i])
        print(f"ADAM_ERR end_to_end/{name}.param: kernel {ek:.4f} torch_fp32 {et:.4f} bound {2 * et + 1:.4f}; "
              f"ours vs torch run directly: {(results['ours'][0][i] - results['torch'][0][i]).abs().max().item():.3e}")
        assert ek <= 2.0 * et + 1.0, f"end_to_end/{name}: err(kernel) = {ek:.4f} > 2 * err(torch fp32) + 1 = {2 * et + 1:.4f}"
    assert results["ours"][2].denom.sum().item() > 0 and results["ours"][2].max_radii2D.max().item() > 0
