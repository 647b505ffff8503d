"""GPU checks of Mip-Splatting's 3D smoothing filter: bags_raster.filter_3D (csrc/filter3d.hip) against its PyTorch statement in
float32 and float64 on the named cases of tests/filter3d_cases.py, its repeatability and order independence; the filtered instance
of the fused activations (csrc/activations.hip) against the float64 statement and float64 autograd; and render() with a filter set
against render() of a plain container whose opacity and scaling are the two PyTorch properties."""
import pytest
import torch

import filter3d_cases as F
from bags_raster import GaussianBag, PipelineParams, filter_3D, filtered_activations_torch
from bags_raster.gaussians import fused_activations
from bags_raster.render import render
from bags_raster.synth import synth_scene
from scenes import make_case, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
CASE_N = [(name, N) for name in F.CASES for N in F.NS]


def _hip(xyz, N, order=None):
    V, K, wh = F.table(N)
    if order is not None:
        V, K, wh = V[order], K[order], wh[order]
    out = filter_3D(xyz.to(DEV), V.to(DEV), K.to(DEV), wh, F.VARIANCE)
    torch.cuda.synchronize()
    return out.cpu()


# ---------------------------------------------------------------------------------------------------------------- 1. filter_3D
@pytest.mark.parametrize("name,N", CASE_N)
def test_filter_against_the_statement(name, N):
    """Every case at every size: each row within 1e-5 (1 + |x|) of the float32 statement -- a row outside it means a validity
    decision went the other way, a defect of the kernel's operation order -- and, off the flip rows, of float64; the rows no camera
    sees equal the statement exactly.

    Measured on an MI355X (the test prints every figure; profiles/filter3d/NOTES.md): bitwise equal to the float32 statement on every
    row of every case, N and size; against float64 at most 1.1e-8 on values of 6e-4 .. 0.11 and 3.2e-5 on `none_valid`'s 285 .. 1138."""
    for P in F.sizes_of(name):
        xyz = F.points(name, N)[:P]
        o32, o64 = F.reference(name, N, F32, P), F.reference(name, N, F64, P)
        out = _hip(xyz, N)
        assert out.shape == (P, 1) and out.dtype == F32 and torch.isfinite(out).all()
        d32 = (out.double() - o32.double()).abs()
        keep = ~F.flips(name, N, P)
        d64 = (out.double() - o64).abs()[keep]
        print("\n%s N=%d P=%d: max |hip - f32| %.3e  |hip - f64| %.3e  bitwise equal to f32 on %d of %d rows"
              % (name, N, P, d32.max().item(), d64.max().item() if d64.numel() else 0.0, int((out == o32).sum()), P))
        assert (d32 <= 1e-5 * (1 + o32.double().abs())).all()
        assert (d64 <= 1e-5 * (1 + o64.abs()[keep])).all()
        if name in ("behind", "none_valid"):
            hidden = ~F.decisions(name, N, F32, P)["any"]
            assert torch.equal(out[hidden], o32[hidden])
            assert name == "behind" or hidden.all()


@pytest.mark.parametrize("name,N", [("ring", 17), ("behind", 70), ("edge", 3), ("max_last", 17), ("max_first", 70), ("none_valid", 1)])
def test_filter_repeats_and_ignores_the_order_of_cameras_and_rows(name, N):
    xyz = F.points(name, N)
    P = xyz.shape[0]
    g = torch.Generator().manual_seed(7 + N)
    first = _hip(xyz, N)
    assert torch.equal(first, _hip(xyz, N))                                                   # two runs
    assert torch.equal(first, _hip(xyz, N, torch.randperm(N, generator=g)))                   # the camera table permuted
    perm = torch.randperm(P, generator=g)
    assert torch.equal(first[perm], _hip(xyz[perm].contiguous(), N))                          # the rows permuted: the cross-block maximum
    assert torch.equal(first.flip(0), _hip(xyz.flip(0).contiguous(), N))


def test_filter_arguments():
    V, K, wh = (t.to(DEV) for t in F.table(3))
    xyz = F.points("ring", 3)[:5].to(DEV)
    assert filter_3D(xyz[:0], V, K, wh).shape == (0, 1)
    out = filter_3D(xyz.requires_grad_(True), V, K, wh)
    assert out.shape == (5, 1) and not out.requires_grad
    xyz = xyz.detach()
    assert torch.equal(out, filter_3D(xyz, V, K, wh.cpu().long()))                            # sizes: any integer dtype, any device
    with pytest.raises(ValueError, match="at least one camera"):
        filter_3D(xyz, V[:0], K[:0], wh[:0])
    for bad in (dict(xyz=xyz[:, :2]), dict(intrinsics=K[:2]), dict(sizes=wh.float()), dict(sizes=wh[:2]), dict(variance=-1.0)):
        a = dict(xyz=xyz, viewmatrices=V, intrinsics=K, sizes=wh)
        a.update(bad)
        with pytest.raises(ValueError, match="filter_3D"):
            filter_3D(**a)
    with pytest.raises(TypeError, match="float32"):
        filter_3D(xyz.double(), V, K, wh)
    with pytest.raises(NotImplementedError, match="filter_3D_torch"):
        filter_3D(xyz, V.cpu(), K, wh)


# ---------------------------------------------------------------------------------------------------------------- 2. filtered activations
def _leaves(P, dtype, device):
    return {n: t.to(device=device, dtype=dtype).clone().requires_grad_(True) for n, t in F.raw(P).items()}


def _backward(op, sc, P, which, device, dtype):
    ct = F.cotangents(P)
    outs = ([op] if which != "scales" else []) + ([sc] if which != "opacity" else [])
    cots = ([ct["opacity"]] if which != "scales" else []) + ([ct["scales"]] if which != "opacity" else [])
    torch.autograd.backward(outs, [c.to(device=device, dtype=dtype) for c in cots])


@pytest.mark.parametrize("kind", F.FILTERS)
@pytest.mark.parametrize("P", F.SIZES)
def test_filtered_activations_against_float64(P, kind):
    """Forward within 1e-5 (1 + |x|) of the float64 statement; every gradient within 1e-4 (scenes.rel_err) of float64 autograd, under
    only g_opacity, only g_scales and both; f = 0 is the unfiltered fused activations within 1e-6 (1 + |x|).

    Measured on an MI355X at P = 1000: 6.0e-8 .. 1.4e-7 for every gradient of `ring` and `huge`."""
    f = F.filter_values(kind, P)
    ref = _leaves(P, F64, "cpu")
    op64, sc64 = filtered_activations_torch(ref["opacity"], ref["scaling"], f.double())
    for which in F.COTANGENTS:
        lv = _leaves(P, F32, DEV)
        shs, op, sc, rot = fused_activations(lv["features_dc"], lv["features_rest"], lv["opacity"], lv["scaling"], lv["rotation"], f.to(DEV))
        assert ((op.detach().cpu().double() - op64.detach()).abs() <= 1e-5 * (1 + op64.detach().abs())).all()
        assert ((sc.detach().cpu().double() - sc64.detach()).abs() <= 1e-5 * (1 + sc64.detach().abs())).all()
        _backward(op, sc, P, which, DEV, F32)
        for t in ref.values():
            t.grad = None
        _backward(*filtered_activations_torch(ref["opacity"], ref["scaling"], f.double()), P, which, "cpu", F64)
        hand = F.by_hand_f64(kind, P, which)
        errs = {}
        for n in ("opacity", "scaling"):
            if ref[n].grad is None:                                   # only g_scales: the raw opacity gets nothing on either side
                assert lv[n].grad is None and which == "scales" and n == "opacity"
                continue
            want = hand[2 if n == "opacity" else 3]
            assert rel_err(ref[n].grad, want) <= 1e-10
            if not want.any():
                # f = 0 under g_opacity alone: dL/d_scaling is exactly zero, and float64 autograd returns its own rounding (1e-17),
                # which is no reference for a relative error; the kernel is held to the exact zero
                assert kind == "zero" and which == "opacity" and n == "scaling" and ref[n].grad.abs().max().item() <= 1e-12
                assert lv[n].grad.abs().max().item() == 0.0
                errs[n] = 0.0
                continue
            errs[n] = rel_err(lv[n].grad, ref[n].grad)
            assert torch.isfinite(lv[n].grad).all() and errs[n] <= 1e-4, (which, n, errs[n])
        print("\n%s P=%d %s:" % (kind, P, which), "  ".join("%s %.2e" % kv for kv in errs.items()))
        assert lv["rotation"].grad is None and lv["features_dc"].grad is None        # unused outputs cost nothing
        if kind == "zero":
            pl = _leaves(P, F32, DEV)
            _, op0, sc0, _ = fused_activations(pl["features_dc"], pl["features_rest"], pl["opacity"], pl["scaling"], pl["rotation"])
            _backward(op0, sc0, P, which, DEV, F32)
            for a, b in ((op, op0), (sc, sc0)) + tuple((lv[n].grad, pl[n].grad) for n in errs):
                b = torch.zeros_like(a) if b is None else b       # only g_opacity: the unfiltered scaling gets no gradient, the filtered one zeros
                assert ((a.detach() - b.detach()).abs() <= 1e-6 * (1 + b.detach().abs())).all()


def test_features_and_rotations_are_those_of_the_unfiltered_launch():
    P = 513
    f = F.filter_values("ring", P).to(DEV)
    a, b = _leaves(P, F32, DEV), _leaves(P, F32, DEV)
    got = fused_activations(a["features_dc"], a["features_rest"], a["opacity"], a["scaling"], a["rotation"], f)
    want = fused_activations(b["features_dc"], b["features_rest"], b["opacity"], b["scaling"], b["rotation"])
    assert torch.equal(got[0], want[0]) and torch.equal(got[3], want[3])
    assert not torch.equal(got[1], want[1]) and not torch.equal(got[2], want[2])
    g = torch.Generator().manual_seed(3)
    cots = [torch.randn(w.shape, generator=g).to(DEV) for w in (want[0], want[3])]
    torch.autograd.backward([got[0], got[3]], cots)
    torch.autograd.backward([want[0], want[3]], cots)
    for n in ("features_dc", "features_rest", "rotation"):
        assert torch.equal(a[n].grad, b[n].grad), n
    with pytest.raises(RuntimeError, match="filter_3D must be"):
        fused_activations(a["features_dc"], a["features_rest"], a["opacity"], a["scaling"], a["rotation"], f[:-1])


def test_bag_without_a_filter_is_as_before_and_with_one_matches_the_properties():
    sc = synth_scene(513, 9, 0.5, 2)
    pc = GaussianBag.from_activated(sc, 2, device=DEV)
    assert pc.filter_3D is None
    for features in (True, False):
        got = pc.activated(features=features)
        want = fused_activations(pc._features_dc if features else None, pc._features_rest if features else None, pc._opacity, pc._scaling, pc._rotation)
        assert got[0] is pc._xyz and all((x is None and y is None) or torch.equal(x, y) for x, y in zip(got[1:], want))
    assert torch.allclose(got[2], pc.get_opacity, rtol=2e-6, atol=1e-7) and torch.allclose(got[3], pc.get_scaling, rtol=2e-6, atol=1e-7)
    V, K, wh = F.table(17)
    f = pc.compute_3D_filter(V.to(DEV), K.to(DEV), wh)
    assert f is pc.filter_3D and f.is_cuda and f.shape == (513, 1)
    assert torch.equal(f, filter_3D(pc._xyz.detach(), V.to(DEV), K.to(DEV), wh, 0.2))
    for features in (True, False):
        xyz, feats, op, scl, rot = pc.activated(features=features)
        for a, b in ((op, pc.get_opacity_with_3D_filter), (scl, pc.get_scaling_with_3D_filter)):
            assert ((a - b).abs() <= 1e-5 * (1 + b.abs())).all()
        assert torch.equal(rot, want[3]) and (feats is None) == (not features)
    pc.filter_3D = f[:-1]
    with pytest.raises(RuntimeError, match="stale.*compute_3D_filter"):
        pc.activated()


# ---------------------------------------------------------------------------------------------------------------- 3. end to end
class _Plain:
    """A container with the reference's properties and nothing else: opacity and scaling are the two PyTorch properties."""

    def __init__(self, bag):
        self._bag = bag
        self.active_sh_degree, self.max_sh_degree = bag.active_sh_degree, bag.max_sh_degree
        self._features_dc, self._features_rest = bag._features_dc, bag._features_rest

    get_xyz = property(lambda self: self._bag.get_xyz)
    get_features = property(lambda self: self._bag.get_features)
    get_rotation = property(lambda self: self._bag.get_rotation)
    get_opacity = property(lambda self: self._bag.get_opacity_with_3D_filter)
    get_scaling = property(lambda self: self._bag.get_scaling_with_3D_filter)


@pytest.mark.parametrize("hybrid", (False, True))
def test_render_picks_the_filter_up(hybrid):
    scene, cam0 = make_case(300, 64, 48, 1.0, 1, seed=5)
    g_img = torch.randn(3, 48, 64, generator=torch.Generator().manual_seed(8)).to(DEV)
    bg = torch.zeros(3, device=DEV)
    from bags_raster.synth import look_at_origin_camera

    def route(kind):
        bag = GaussianBag.from_activated(scene, 1, device=DEV)
        cam = look_at_origin_camera(64, 48, device=DEV)
        if kind != "unfiltered":
            view, _, intr, _ = cam.get_matrices(None, None)
            bag.compute_3D_filter(view.detach()[None], intr.detach()[None], torch.tensor([[64, 48]]))
        res = render(cam, _Plain(bag) if kind == "plain" else bag, PipelineParams(), bg, 0.0, None, hybrid=hybrid)
        (res["render"] * g_img).sum().backward()
        torch.cuda.synchronize()
        return res["render"].detach(), [t.grad for t in bag.leaves()], bag
    img, grads, bag = route("fused")
    want, want_grads, _ = route("plain")
    plain, _, _ = route("unfiltered")
    assert (bag.filter_3D > 0.01).all() and bag.filter_3D.shape == (300, 1)
    assert ((img - want).abs() <= 1e-5 * (1 + want.abs())).all(), (img - want).abs().max().item()
    assert (img - plain).abs().max().item() > 1e-3                                          # the filter is seen
    errs = [rel_err(a, b) for a, b in zip(grads, want_grads)]
    print("\nleaf gradients, fused against the PyTorch properties:", errs)
    assert all(a is not None and b is not None for a, b in zip(grads, want_grads)) and max(errs) <= 1e-4, errs
    with pytest.raises(NotImplementedError, match="compute_cov3D_python"):
        render(look_at_origin_camera(64, 48, device=DEV), bag, PipelineParams(compute_cov3D_python=True), bg, 0.0, None, hybrid=hybrid)
