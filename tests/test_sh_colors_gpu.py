"""bags_raster.sh_colors (csrc/sh_colors.hip) against ``_python_colors`` restated in float64, and inside ``render()``.

Bar (the rule of tests/loss_cases.py): the kernel's error against the float64 reference -- colours by max-abs, each gradient by
relative L2 -- is at most FACTOR x the error the float32 ``_python_colors`` (PyTorch, same GPU, same input) has against the same
reference, and never asked to be below FLOOR = 16 float32 epsilons, the reordering slack of a 16-term sum.  Nothing in the bar
comes from the kernel.  Elements whose float64 ``raw`` lies within NEAR of zero are left out (their clamp decision may
legitimately differ in float32); at most MAX_LEFT_OUT per case.
"""
import functools
import importlib
from types import SimpleNamespace

import pytest
import torch

from bags_raster import sh_colors
from bags_raster.gaussians import RGB2SH, eval_sh
from scenes import make_case, rel_err

pytestmark = pytest.mark.gpu

FACTOR = 4.0
FLOOR = 16 * torch.finfo(torch.float32).eps
NEAR = 1e-5
MAX_LEFT_OUT = 2
CAMPOS = (0.3, -0.2, 4.0)
CASES = [(P, maxdeg, deg, seed) for P in (1, 255, 257, 1025) for maxdeg in range(4) for deg in range(maxdeg + 1) for seed in (0, 1)]
NAMES = ("dc", "rest", "xyz", "campos")


def make_inputs(P, maxdeg, deg, seed):
    g = torch.Generator().manual_seed(1000 * P + 10 * maxdeg + deg + 100 * seed)
    K = (maxdeg + 1) ** 2
    xyz = torch.rand(P, 3, generator=g) * 2.6 - 1.3
    dc = RGB2SH(torch.rand(P, 1, 3, generator=g))
    dc[1::3] -= 2.0                        # all channels clamp
    dc[2::3, :, 1] -= 1.0                  # one channel straddles the clamp
    rest = 0.3 * torch.randn(P, K - 1, 3, generator=g)
    campos = torch.tensor(CAMPOS)
    cot = torch.randn(P, 3, generator=g)
    cot[2::5] = 0.0                        # the rasterizer's culled rows
    return dc, rest, xyz, campos, cot


def python_route(deg, maxdeg, dc, rest, xyz, campos, cot):
    """``render._python_colors`` on leaves of the given dtype / device: raw, rgb and the four gradients (zeros where autograd has none)."""
    R = importlib.import_module("bags_raster.render")
    leaves = [t.clone().requires_grad_(True) for t in (dc, rest, xyz, campos)]
    pc = SimpleNamespace(max_sh_degree=maxdeg, active_sh_degree=deg)
    feats = torch.cat((leaves[0], leaves[1]), dim=1)
    rgb = R._python_colors(pc, leaves[2], feats, leaves[3], 0.0)
    rgb.backward(cot)
    with torch.no_grad():
        u = xyz - campos
        u = u / u.norm(dim=1, keepdim=True)
        raw = eval_sh(deg, feats.transpose(1, 2), u) + 0.5
    return raw.detach(), rgb.detach(), [torch.zeros_like(t) if t.grad is None else t.grad for t in leaves]


def kernel_route(deg, dc, rest, xyz, campos, cot, split, only=None):
    """sh_colors on the GPU, packed or split; ``only``: index of the single leaf that requires a gradient."""
    leaves = [t.clone().requires_grad_(only is None or only == k) for k, t in enumerate((dc, rest, xyz, campos))]
    if split:
        rgb = sh_colors(deg, leaves[0], leaves[2], leaves[3], shs_rest=leaves[1])
    else:
        rgb = sh_colors(deg, torch.cat((leaves[0], leaves[1]), dim=1), leaves[2], leaves[3])
    rgb.backward(cot, retain_graph=True)
    first = [None if t.grad is None else t.grad.clone() for t in leaves]
    for t in leaves:
        t.grad = None
    rgb.backward(cot)                                                    # the same graph again: the same bits
    second = [None if t.grad is None else t.grad.clone() for t in leaves]
    return rgb.detach(), first, second


@functools.lru_cache(maxsize=None)
def case(P, maxdeg, deg, seed):
    cpu = make_inputs(P, maxdeg, deg, seed)
    raw64, rgb64, g64 = python_route(deg, maxdeg, *[t.double() for t in cpu])
    dev = [t.cuda() for t in cpu]
    _, rgb32, g32 = python_route(deg, maxdeg, *dev)
    packed = kernel_route(deg, *dev, split=False)
    split = kernel_route(deg, *dev, split=True) if maxdeg > 0 else None         # K = 1 has no rest tensor to split off
    return dict(cpu=cpu, dev=dev, raw64=raw64, rgb64=rgb64, g64=g64, rgb32=rgb32.cpu(), g32=[g.cpu() for g in g32], packed=packed, split=split)


def _rel_l2(a, b, keep=None):
    a, b = a.double(), b.double()
    if keep is not None:
        a, b = a[keep], b[keep]
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("P,maxdeg,deg,seed", CASES)
def test_values_and_gradients_against_float64(P, maxdeg, deg, seed):
    c = case(P, maxdeg, deg, seed)
    near = c["raw64"].abs() < NEAR                                       # (P,3) elements left out
    assert int(near.sum()) <= MAX_LEFT_OUT, int(near.sum())
    keep_el = ~near
    keep_row = ~near.any(dim=1)
    K = (maxdeg + 1) ** 2
    keeps = {"dc": keep_el.unsqueeze(1), "rest": keep_el.unsqueeze(1).expand(P, K - 1, 3), "xyz": keep_row.unsqueeze(1).expand(P, 3), "campos": None}
    if P == 1025:
        frac = (c["raw64"] < 0).double().mean().item()
        assert 0.2 <= frac <= 0.3, frac                                  # the generator's clamped share (0.213 .. 0.293 over the cases)
    for layout in ("packed", "split"):
        if c[layout] is None:
            continue
        rgb, grads, _ = c[layout]
        err = (rgb.cpu().double() - c["rgb64"])[keep_el].abs().max().item() if keep_el.any() else 0.0
        err32 = (c["rgb32"].double() - c["rgb64"])[keep_el].abs().max().item() if keep_el.any() else 0.0
        print(f"{layout} P={P} K={K} deg={deg} seed={seed} colours: kernel {err:.3e} pytorch32 {err32:.3e}")
        assert err <= max(FACTOR * err32, FLOOR), (layout, err, err32)
        for k, name in enumerate(NAMES):
            if name == "rest" and K == 1:
                continue
            ref, got, py = c["g64"][k], grads[k].cpu(), c["g32"][k]
            keep = keeps[name]
            if (ref if keep is None else ref[keep]).norm().item() == 0.0:       # degree 0 direction gradients, P = 1 culled ...: exact zeros
                assert not (got if keep is None else got[keep]).any(), (layout, name)
                continue
            e, e32 = _rel_l2(got, ref, keep), _rel_l2(py, ref, keep)
            print(f"{layout} P={P} K={K} deg={deg} seed={seed} d{name}: kernel {e:.3e} pytorch32 {e32:.3e}")
            assert e <= max(FACTOR * e32, FLOOR), (layout, name, e, e32)


@pytest.mark.parametrize("P,maxdeg,deg,seed", CASES)
def test_exact_properties(P, maxdeg, deg, seed):
    c = case(P, maxdeg, deg, seed)
    dc, rest, xyz, campos, cot = c["dev"]
    K, nb = (maxdeg + 1) ** 2, (deg + 1) ** 2
    rgb, g, g_again = c["packed"]
    same = lambda a, b: (a is None and b is None) or torch.equal(a, b)
    # backward twice: the same bits, campos included
    for a, b in zip(g, g_again):
        assert same(a, b)
    # packed and split layouts: identical colours and gradients
    if c["split"] is not None:
        rgb_s, gs, gs_again = c["split"]
        assert torch.equal(rgb, rgb_s)
        for a, b in zip(g, gs):
            assert same(a, b)
        for a, b in zip(gs, gs_again):
            assert same(a, b)
    g_dc, g_rest, g_xyz, g_campos = g
    g_sh = g_dc if K == 1 else torch.cat((g_dc, g_rest), dim=1)
    # rows with a zero cotangent: all-zero SH and xyz gradients
    culled = (cot == 0).all(dim=1)
    assert not g_sh[culled].any() and not g_xyz[culled].any()
    # stored rows beyond the active degree
    assert not g_sh[:, nb:].any()
    # a fully clamped Gaussian (float64 raw clearly below zero in all channels) has zero gradients
    full = (c["raw64"] < -NEAR).all(dim=1).cuda()
    if P >= 255:
        assert full.any()
    assert not rgb[full].any() and not g_sh[full].any() and not g_xyz[full].any()
    # degree 0: no direction, no xyz / campos gradient
    if deg == 0:
        assert not g_xyz.any() and not g_campos.any()
    # one gradient alone: the bits it has when all four are asked for
    for split in ((False, True) if maxdeg > 0 else (False,)):
        for k in range(4):
            if k == 1 and K == 1:
                continue
            _, alone, _ = kernel_route(deg, dc, rest, xyz, campos, cot, split=split, only=k)
            assert [x is not None for x in alone] == [j == k for j in range(4)], (split, k)
            assert torch.equal(alone[k], g[k]), (split, NAMES[k])


def test_render_hybrid_path_is_fused_and_matches_python_colors(monkeypatch):
    """render(hybrid=True) on a GaussianBag: colours from sh_colors fed with the split leaves (no torch.cat of the features),
    image and every leaf / pose gradient equal to the same call with ``_python_colors`` in its place, within the bars of
    test_render_caller_paths_agree_and_match_oracle."""
    from bags_raster.gaussians import GaussianBag
    from bags_raster.render import render, PipelineParams
    from bags_raster.synth import sphere_views
    R = importlib.import_module("bags_raster.render")
    dev = "cuda"
    P, W, H = 1500, 160, 128
    scene, _ = make_case(P, W, H, 1.5, 3, seed=17)
    cam = sphere_views(3, W, H, noise=0.05, device=dev)[2]
    gimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
    bgc = torch.tensor([0.2, 0.1, 0.3], device=dev)

    feature_cats = []
    real_cat = torch.cat

    def counting_cat(tensors, *args, **kwargs):
        ts = list(tensors)
        if any(t.dim() == 3 and t.shape[0] == P and t.shape[-1] == 3 for t in ts):
            feature_cats.append([tuple(t.shape) for t in ts])
        return real_cat(ts, *args, **kwargs)

    fused_calls = []
    real_sh_colors = R.sh_colors

    def spying_sh_colors(deg, shs, xyz, campos, shs_rest=None):
        fused_calls.append((tuple(shs.shape), None if shs_rest is None else tuple(shs_rest.shape)))
        return real_sh_colors(deg, shs, xyz, campos, shs_rest=shs_rest)

    def run(substitute):
        pc = GaussianBag.from_activated(scene, 3, device=dev)
        for p_ in cam.pose_leaves():
            p_.grad = None
        if substitute:
            def python_colors(deg, shs, xyz, campos, shs_rest=None):
                assert deg == pc.active_sh_degree
                feats = shs if shs_rest is None else real_cat((shs, shs_rest), dim=1)
                return R._python_colors(pc, xyz, feats, campos, 0.0)
            monkeypatch.setattr(R, "sh_colors", python_colors)
        else:
            monkeypatch.setattr(R, "sh_colors", spying_sh_colors)
        monkeypatch.setattr(torch, "cat", counting_cat)
        out = render(cam, pc, PipelineParams(), bgc, 0.0, None, scaling_modifier=0.9)
        out["render"].backward(gimg)
        monkeypatch.undo()
        return dict(img=out["render"].detach().cpu(), radii=out["radii"].cpu(),
                    grads=[t.grad.detach().cpu().clone() for t in pc.leaves()] + [t.grad.detach().cpu().clone() for t in cam.pose_leaves()] +
                          [out["viewspace_points"].grad.detach().cpu(), out["viewspace_points_densify"].grad.detach().cpu()])

    fused = run(False)
    assert fused_calls == [((P, 1, 3), (P, 15, 3))], fused_calls          # the leaves as stored
    assert feature_cats == [], feature_cats                               # no concatenation of the features anywhere in the call
    ref = run(True)
    assert torch.equal(fused["radii"], ref["radii"])
    assert (fused["img"] - ref["img"]).abs().max().item() < 2e-5
    for a, b in zip(fused["grads"], ref["grads"]):
        assert rel_err(a, b) < 2e-4, rel_err(a, b)
