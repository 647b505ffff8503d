"""bags_raster.sh_colors_views (csrc/sh_colors.hip, the multi-view kernels) and render_views on the GPU.

Three yardsticks, none of them taken from the kernels under test:
  * forward: view v's colours are the bits of the single-view ``sh_colors`` for ``campos_v``;
  * backward, exact: the gradients of the coefficients and of ``xyz`` are the bits of the fp32 fold ((g_0 + g_1) + g_2) ... of the
    single-view kernel's gradients over the views a loss uses, in view order;
  * backward, float64: ``_python_colors`` in float64 summed over the views, by the rule and the constants of
    tests/test_sh_colors_gpu.py (kernel error <= max(FACTOR x the float32 PyTorch route's own error, FLOOR); colours by max-abs,
    gradients by relative L2, dL/dcampos per view).  Elements whose float64 ``raw`` lies within NEAR of zero in some view are left
    out, at most MAX_LEFT_OUT per view of a case: the inputs below were chosen on the CPU, with the float64 reference alone, to
    stay within that cap (SEED_OF holds the cases that needed another seed than 0), and the cap is asserted.

Per view the cotangent zeroes rows (2 + v)::5 (the rows the rasterizer culled in that view) and, in every view, rows 7::11 (culled
everywhere: Gaussians without a contributing view).  Where V >= 2 view 1's cotangent is all zero; where V >= 5 no loss uses view 3.
"""
import functools
import importlib
import math
from types import SimpleNamespace

import pytest
import torch

from bags_raster import _lib, sh_colors, sh_colors_views
from bags_raster.gaussians import eval_sh
from scenes import make_case
from test_sh_colors_gpu import FACTOR, FLOOR, MAX_LEFT_OUT, NEAR, _rel_l2, make_inputs

pytestmark = pytest.mark.gpu

PS = (1, 255, 257, 1025)
FULL_CROSS = [(maxdeg, deg) for maxdeg in range(4) for deg in range(maxdeg + 1)]
CASES = ([(P, 5, maxdeg, deg) for P in PS for maxdeg, deg in FULL_CROSS] +
         [(P, V, maxdeg, deg) for P in PS for V in (1, 2, 16) for maxdeg, deg in ((3, 3), (3, 1), (0, 0))])
SEED_OF = {}                     # (P, V, maxdeg, deg) -> seed, where seed 0 leaves more than MAX_LEFT_OUT elements of a view out
ZERO_VIEW, UNUSED_VIEW = 1, 3


def make_view_inputs(P, V, maxdeg, deg):
    """make_inputs' Gaussians, V camera centres spread over a shell around the cloud, V cotangents; ``used``: views a loss depends on."""
    seed = SEED_OF.get((P, V, maxdeg, deg), 0)
    dc, rest, xyz, _, _ = make_inputs(P, maxdeg, deg, seed)
    g = torch.Generator().manual_seed(77_000 + 1000 * P + 100 * V + 10 * maxdeg + deg + 7 * seed)
    k = torch.arange(V, dtype=torch.float64) + 0.5
    z = 1.0 - 2.0 * k / V                                                    # a golden spiral: distinct directions all around
    phi = k * (math.pi * (3.0 - math.sqrt(5.0))) + float(torch.rand(1, generator=g, dtype=torch.float64)) * 2 * math.pi
    radius = 3.5 + torch.rand(V, generator=g, dtype=torch.float64)           # the cloud lies in [-1.3, 1.3]^3
    s = (1.0 - z * z).sqrt()
    centres = (torch.stack((s * phi.cos(), s * phi.sin(), z), dim=1) * radius[:, None]).float()
    cots = []
    for v in range(V):
        cot = torch.randn(P, 3, generator=g)
        cot[(2 + v)::5] = 0.0
        cot[7::11] = 0.0
        if V >= 2 and v == ZERO_VIEW:
            cot.zero_()
        cots.append(cot)
    used = [not (V >= 5 and v == UNUSED_VIEW) for v in range(V)]
    return dc, rest, xyz, [centres[v].clone() for v in range(V)], cots, used


def python_views(deg, maxdeg, dc, rest, xyz, centres, cots, used):
    """``render._python_colors`` per view on leaves of the inputs' dtype / device, one backward over the used views: raw and rgb per
    view, the summed gradients of dc / rest / xyz and each view's dL/dcampos (zeros where autograd has none)."""
    R = importlib.import_module("bags_raster.render")
    leaves = [t.clone().requires_grad_(True) for t in (dc, rest, xyz)]
    cams = [c.clone().requires_grad_(True) for c in centres]
    pc = SimpleNamespace(max_sh_degree=maxdeg, active_sh_degree=deg)
    feats = torch.cat((leaves[0], leaves[1]), dim=1)
    rgbs = [R._python_colors(pc, leaves[2], feats, c, 0.0) for c in cams]
    torch.autograd.backward([r for r, u in zip(rgbs, used) if u], [c for c, u in zip(cots, used) if u])
    raws = []
    with torch.no_grad():
        for c in centres:
            u = xyz - c
            raws.append(eval_sh(deg, feats.transpose(1, 2), u / u.norm(dim=1, keepdim=True)) + 0.5)
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return raws, [r.detach() for r in rgbs], [zero(t) for t in leaves], [zero(c) for c in cams]


def kernel_views(deg, dc, rest, xyz, centres, cots, used, split, only=None):
    """sh_colors_views, packed or split.  ``only``: 0 dc, 1 rest, 2 xyz, 3 + v campos_v -- the single leaf that requires a gradient
    (packed: dc and rest are one tensor, either index asks for it).  Returns rgb, the gradients and those of a second backward."""
    want = lambda k: only is None or only == k
    cams = [c.clone().requires_grad_(want(3 + v)) for v, c in enumerate(centres)]
    xyz_l = xyz.clone().requires_grad_(want(2))
    if split:
        sh = [dc.clone().requires_grad_(want(0)), rest.clone().requires_grad_(want(1))]
        rgbs = sh_colors_views(deg, sh[0], xyz_l, cams, shs_rest=sh[1])
    else:
        sh = [torch.cat((dc, rest), dim=1).requires_grad_(want(0) or want(1))]
        rgbs = sh_colors_views(deg, sh[0], xyz_l, cams)
    leaves = sh + [xyz_l] + cams
    outs, gs = [r for r, u in zip(rgbs, used) if u], [c for c, u in zip(cots, used) if u]
    grads = []
    for again in (False, True):
        for t in leaves:
            t.grad = None
        torch.autograd.backward(outs, gs, retain_graph=not again)
        grads.append([None if t.grad is None else t.grad.clone() for t in leaves])
    return [r.detach() for r in rgbs], grads[0], grads[1]


def single_view_fold(deg, dc, rest, xyz, centres, cots, used, split):
    """The single-view kernel per view, its colours, and the fp32 fold of its gradients over the used views in view order."""
    rgbs, fold, g_cam = [], None, []
    for c, cot, u in zip(centres, cots, used):
        cam = c.clone().requires_grad_(True)
        xyz_l = xyz.clone().requires_grad_(True)
        if split:
            sh = [dc.clone().requires_grad_(True), rest.clone().requires_grad_(True)]
            rgb = sh_colors(deg, sh[0], xyz_l, cam, shs_rest=sh[1])
        else:
            sh = [torch.cat((dc, rest), dim=1).requires_grad_(True)]
            rgb = sh_colors(deg, sh[0], xyz_l, cam)
        rgbs.append(rgb.detach())
        if not u:
            g_cam.append(None)
            continue
        rgb.backward(cot)
        g = [t.grad for t in sh + [xyz_l]]
        fold = g if fold is None else [a + b for a, b in zip(fold, g)]
        g_cam.append(cam.grad)
    return rgbs, fold, g_cam


@functools.lru_cache(maxsize=None)
def case(P, V, maxdeg, deg):
    dc, rest, xyz, centres, cots, used = make_view_inputs(P, V, maxdeg, deg)
    dbl = lambda ts: [t.double() for t in ts]
    raw64, rgb64, g64, gc64 = python_views(deg, maxdeg, dc.double(), rest.double(), xyz.double(), dbl(centres), dbl(cots), used)
    dev = lambda ts: [t.cuda() for t in ts]
    d = dict(dc=dc.cuda(), rest=rest.cuda(), xyz=xyz.cuda(), centres=dev(centres), cots=dev(cots), used=used)
    _, rgb32, g32, gc32 = python_views(deg, maxdeg, **d)
    layouts = (False, True) if maxdeg > 0 else (False,)                   # K = 1 has no rest tensor to split off
    return dict(d=d, raw64=raw64, rgb64=rgb64, g64=g64, gc64=gc64, rgb32=[t.cpu() for t in rgb32], g32=[t.cpu() for t in g32],
                gc32=[t.cpu() for t in gc32], kernel={s: kernel_views(deg, split=s, **d) for s in layouts},
                single={s: single_view_fold(deg, split=s, **d) for s in layouts})


def _sh_grads(grads, split, K):
    """(dc, rest, xyz, [campos_v]) from kernel_views' gradient list, the packed tensor cut in two."""
    if split:
        return grads[0], grads[1], grads[2], grads[3:]
    return grads[0][:, :1], grads[0][:, 1:], grads[1], grads[2:]


@pytest.mark.parametrize("P,V,maxdeg,deg", CASES)
def test_forward_is_the_single_view_kernel_per_view(P, V, maxdeg, deg):
    c = case(P, V, maxdeg, deg)
    for split, (rgbs, _, _) in c["kernel"].items():
        assert len(rgbs) == V
        for v in range(V):
            assert rgbs[v].shape == (P, 3)
            assert torch.equal(rgbs[v], c["single"][split][0][v]), (split, v)
            assert torch.equal(rgbs[v], c["single"][False][0][v]), (split, v)      # ... and packed or split, the same bits
    if P == 1025 and deg > 0 and V >= 2:                                   # the views do see different clamp decisions
        masks = torch.stack([r < 0 for r in c["raw64"]])
        assert (masks != masks[0]).any()


@pytest.mark.parametrize("P,V,maxdeg,deg", CASES)
def test_backward_is_the_fold_of_the_single_view_gradients(P, V, maxdeg, deg):
    c = case(P, V, maxdeg, deg)
    d = c["d"]
    K, nb = (maxdeg + 1) ** 2, (deg + 1) ** 2
    same = lambda a, b: (a is None and b is None) or (a is not None and b is not None and torch.equal(a, b))
    contributing = torch.zeros(P, dtype=torch.bool, device="cuda")
    for cot, u in zip(d["cots"], d["used"]):
        if u:
            contributing |= (cot != 0).any(dim=1)
    if P >= 255:
        assert (~contributing).any() and contributing.any()
    for split, (_, grads, again) in c["kernel"].items():
        fold = c["single"][split][1]
        n_sh = 2 if split else 1
        for k in range(n_sh + 1):                                          # coefficients and xyz: the fold's bits
            assert torch.equal(grads[k], fold[k]), (split, k)
        g_dc, g_rest, g_xyz, g_cams = _sh_grads(grads, split, K)
        g_sh = torch.cat((g_dc, g_rest), dim=1)
        assert not g_sh[:, nb:].any()                                      # stored rows beyond the active degree
        assert not g_sh[~contributing].any() and not g_xyz[~contributing].any()
        if deg == 0:
            assert not g_xyz.any() and not any(g.any() for g in g_cams)
        for a, b in zip(grads, again):                                     # the same graph again: the same bits
            assert same(a, b), split
        _, fresh, _ = kernel_views(deg, split=split, **d)                  # a fresh run: the same bits
        for a, b in zip(grads, fresh):
            assert same(a, b), split
        n = len(grads)
        for only in ((0, 1, 2, 3, 3 + V - 1) if split else (0, 2, 3, 3 + V - 1)):       # one leaf alone: its bits of the all-leaves run
            _, alone, _ = kernel_views(deg, split=split, only=only, **d)
            at = only if split else max(only - 1, 0)
            assert [x is not None for x in alone] == [j == at for j in range(n)], (split, only)
            assert torch.equal(alone[at], grads[at]), (split, only)
    if len(c["kernel"]) == 2:                                              # packed and split: identical gradients
        a, b = _sh_grads(c["kernel"][False][1], False, K), _sh_grads(c["kernel"][True][1], True, K)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        for x, y in zip(a[3], b[3]):
            assert torch.equal(x, y)


@pytest.mark.parametrize("P,V,maxdeg,deg", CASES)
def test_values_and_gradients_against_float64(P, V, maxdeg, deg):
    c = case(P, V, maxdeg, deg)
    K = (maxdeg + 1) ** 2
    near_v = [r.abs() < NEAR for r in c["raw64"]]
    for v, n in enumerate(near_v):
        assert int(n.sum()) <= MAX_LEFT_OUT, (v, int(n.sum()))              # the cap, per view of the case
    near = torch.stack(near_v).any(dim=0)
    keep_el, keep_row = ~near, ~near.any(dim=1)
    keeps = [keep_el.unsqueeze(1), keep_el.unsqueeze(1).expand(P, K - 1, 3), keep_row.unsqueeze(1).expand(P, 3)]
    tag = f"P={P} V={V} K={K} deg={deg}"

    def check(what, got, ref, py, keep):
        if (ref if keep is None else ref[keep]).norm().item() == 0.0:      # no direction at degree 0, a view without a cotangent ...
            assert got is None or not (got if keep is None else got[keep]).any(), what
            return
        e, e32 = _rel_l2(got, ref, keep), _rel_l2(py, ref, keep)
        print(f"{tag} {what}: kernel {e:.3e} pytorch32 {e32:.3e}")
        assert e <= max(FACTOR * e32, FLOOR), (what, e, e32)

    for split, (rgbs, grads, _) in c["kernel"].items():
        name = "split" if split else "packed"
        for v in range(V):
            k_el = ~near_v[v]
            err = (rgbs[v].cpu().double() - c["rgb64"][v])[k_el].abs().max().item() if k_el.any() else 0.0
            err32 = (c["rgb32"][v].double() - c["rgb64"][v])[k_el].abs().max().item() if k_el.any() else 0.0
            print(f"{tag} {name} colours view {v}: kernel {err:.3e} pytorch32 {err32:.3e}")
            assert err <= max(FACTOR * err32, FLOOR), (name, v, err, err32)
        g_dc, g_rest, g_xyz, g_cams = _sh_grads(grads, split, K)
        for k, (what, got) in enumerate((("ddc", g_dc), ("drest", g_rest), ("dxyz", g_xyz))):
            if what == "drest" and K == 1:
                continue
            check(f"{name} {what}", got.cpu(), c["g64"][k], c["g32"][k], keeps[k])
        for v in range(V):
            check(f"{name} dcampos[{v}]", None if g_cams[v] is None else g_cams[v].cpu(), c["gc64"][v], c["gc32"][v], None)


# ---------------------------------------------------------------------------------------------- render_views
OUT_KEYS = ("render", "radii", "depth", "weights", "means2D", "visibility_filter", "viewspace_points", "viewspace_points_densify")


@functools.lru_cache(maxsize=None)
def _scene():
    from bags_raster.synth import sphere_views
    P, W, H = 1500, 160, 128
    scene, _ = make_case(P, W, H, 1.5, 3, seed=17)
    cams = sphere_views(3, W, H, noise=0.05, device="cuda")
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand(3, H, W, generator=g).cuda() for _ in cams]
    return scene, cams, gts, torch.tensor([0.2, 0.1, 0.3], device="cuda")


def _fresh(scene, cams):
    from bags_raster.gaussians import GaussianBag
    for cam in cams:
        for p_ in cam.pose_leaves():
            p_.grad = None
    return GaussianBag.from_activated(scene, 3, device="cuda")


def test_render_views_matches_render_and_makes_one_colour_launch(monkeypatch):
    from bags_raster.loss import fused_photometric_loss
    from bags_raster.render import PipelineParams, render, render_views
    scene, cams, gts, bg = _scene()
    kw = dict(scaling_modifier=0.9)

    per_view, outs_single = [], []
    for cam, gt in zip(cams, gts):                                        # each view alone through render(), .grad cleared between
        pc = _fresh(scene, cams)
        out = render(cam, pc, PipelineParams(), bg, 0.0, None, **kw)
        fused_photometric_loss(out["render"], gt).backward()
        outs_single.append({k: out[k].detach().clone() for k in OUT_KEYS})
        per_view.append([t.grad.clone() for t in pc.leaves()] + [None if t.grad is None else t.grad.clone() for c in cams for t in c.pose_leaves()])

    names = []
    real_call = _lib.call

    def spying_call(name, *args):
        names.append(name)
        return real_call(name, *args)

    pc = _fresh(scene, cams)
    monkeypatch.setattr(_lib, "call", spying_call)
    outs = render_views(cams, pc, PipelineParams(), bg, 0.0, None, **kw)
    monkeypatch.undo()
    assert names.count("bags_sh_colors_views_forward") == 1 and names.count("bags_sh_colors_forward") == 0, names
    assert isinstance(outs, list) and len(outs) == len(cams)
    for out, ref in zip(outs, outs_single):
        assert set(out) == set(OUT_KEYS)
        for k in OUT_KEYS:
            assert torch.equal(out[k].detach(), ref[k]), k
    sum(fused_photometric_loss(out["render"], gt) for out, gt in zip(outs, gts)).backward()
    got = [t.grad for t in pc.leaves()] + [t.grad for c in cams for t in c.pose_leaves()]

    eps16 = 16 * torch.finfo(torch.float32).eps
    for k, g in enumerate(got):
        parts = [pv[k] for pv in per_view if pv[k] is not None]
        ref = sum(p.double() for p in parts)                               # float64 sum: the reference
        seq = parts[0]
        for p in parts[1:]:
            seq = seq + p                                                  # fp32 fold: the sequential route, as autograd accumulates
        e, e_seq = _rel_l2(g, ref), _rel_l2(seq, ref)
        print(f"leaf {k}: render_views {e:.3e} sequential {e_seq:.3e}")
        assert e <= max(4.0 * e_seq, eps16), (k, e, e_seq)


@pytest.mark.parametrize("path", ["raster_sh", "override_color"])
def test_render_views_other_colour_paths_are_render_per_camera(path):
    from bags_raster.render import PipelineParams, render, render_views
    scene, cams, _, bg = _scene()
    pc = _fresh(scene, cams)
    kw = dict(scaling_modifier=0.9, hybrid=False)
    if path == "override_color":
        kw["override_color"] = torch.rand(pc.get_xyz.shape[0], 3, generator=torch.Generator().manual_seed(9)).cuda()
    with torch.no_grad():
        outs = render_views(cams, pc, PipelineParams(), bg, 0.0, None, **kw)
        assert len(outs) == len(cams)
        for cam, out in zip(cams, outs):
            ref = render(cam, pc, PipelineParams(), bg, 0.0, None, **kw)
            for k in OUT_KEYS:
                assert torch.equal(out[k], ref[k]), (path, k)
