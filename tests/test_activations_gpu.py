"""Fused parameter activations (csrc/activations.hip behind bags_activations_forward / _backward) against the PyTorch
properties of GaussianBag, which tests/test_golden_cpu.py pins to the reference (scene/gaussian_model.py:118-141)."""
import pytest
import torch

from bags_raster.gaussians import GaussianBag, fused_activations
from bags_raster.synth import synth_scene

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("P,deg", [(1000, 3), (257, 0), (1, 2)])
def test_fused_activations_match_properties(P, deg):
    sc = synth_scene(P, 9, 0.5, deg)
    g = torch.Generator().manual_seed(2)
    sc["rotations"] = sc["rotations"] * (0.3 + 2.0 * torch.rand(P, 1, generator=g))        # un-normalised quaternions
    pc0 = GaussianBag.from_activated(sc, deg, device=DEV)
    pc1 = GaussianBag.from_activated(sc, deg, device=DEV)
    with torch.no_grad():
        for a, b in zip(pc0.leaves(), pc1.leaves()):
            b.copy_(a)
        pc0._rotation.copy_(sc["rotations"].to(DEV)); pc1._rotation.copy_(sc["rotations"].to(DEV))
    want = [pc0.get_xyz, pc0.get_features, pc0.get_opacity, pc0.get_scaling, pc0.get_rotation]
    got = list(pc1.activated())
    cots = [torch.randn(w.shape, generator=g).to(DEV) for w in want]
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.allclose(a, b, rtol=2e-6, atol=1e-7), (a - b).abs().max()
    torch.autograd.backward(want[1:], cots[1:])
    torch.autograd.backward(got[1:], cots[1:])
    for a, b in zip(pc1.leaves()[1:], pc0.leaves()[1:]):
        if a.numel() == 0:                                  # degree 0: features_rest is (P,0,3)
            continue
        assert a.grad is not None and torch.allclose(a.grad, b.grad, rtol=1e-4, atol=1e-5), (a.grad - b.grad).abs().max()   # (g - q (q.g)) / |q| cancels


def test_fused_activations_partial_use_and_errors():
    sc = synth_scene(300, 1, 0.5, 3)
    pc = GaussianBag.from_activated(sc, 3, device=DEV)
    _, shs, op, scl, rot = pc.activated()
    (scl.sum() + op.sum()).backward()                     # shs and rotations unused: their leaves get no gradient
    assert pc._features_dc.grad is None and pc._features_rest.grad is None and pc._rotation.grad is None
    assert torch.allclose(pc._scaling.grad, torch.exp(pc._scaling.detach()))
    with pytest.raises(RuntimeError, match="GPU"):
        fused_activations(torch.zeros(2, 1, 3), torch.zeros(2, 15, 3), torch.zeros(2, 1), torch.zeros(2, 3), torch.ones(2, 4))



def test_activations_without_the_feature_concatenation():
    """activated(features=False): the three activations from one launch with one thread per Gaussian, no (P,K,3) tensor."""
    sc = synth_scene(500, 4, 0.5, 3)
    pc0 = GaussianBag.from_activated(sc, 3, device=DEV)
    pc1 = GaussianBag.from_activated(sc, 3, device=DEV)
    want, got = list(pc0.activated()), list(pc1.activated(features=False))
    assert got[1] is None
    g = torch.Generator().manual_seed(6)
    for j in (2, 3, 4):
        assert torch.equal(got[j], want[j])
    cots = [torch.randn(w.shape, generator=g).to(DEV) for w in want]
    torch.autograd.backward(want[2:], cots[2:]); torch.autograd.backward(got[2:], cots[2:])
    for a, b in zip(pc1.leaves()[3:], pc0.leaves()[3:]):
        assert torch.equal(a.grad, b.grad)
    assert pc1._features_dc.grad is None and pc1._features_rest.grad is None


def test_fused_activations_at_edge_values():
    """Saturated sigmoid and exp inputs, and quaternions at and around the 1e-12 clamp of normalize (zero, norms 1e-13 and
    5e-13 below it, 2e-12 just above it, and a single component of 1e-20 whose square underflows), in the first rows of a
    257-Gaussian set: forward against GaussianBag's properties, backward against their autograd, nothing NaN where PyTorch is
    finite.  The clamped rows have gradients of ~1e12 and exp(88) of ~1e38, so beside the whole-tensor bar (rtol 1e-4, atol
    1e-5 of the largest reference gradient) the untouched rows are held to the absolute bar of
    test_fused_activations_match_properties."""
    P, deg = 257, 1
    sc = synth_scene(P, 9, 0.5, deg)
    g = torch.Generator().manual_seed(4)
    sc["rotations"] = sc["rotations"] * (0.3 + 2.0 * torch.rand(P, 1, generator=g))
    pc0 = GaussianBag.from_activated(sc, deg, device=DEV)
    pc1 = GaussianBag.from_activated(sc, deg, device=DEV)
    raw_op = torch.tensor([-104.0, -90.0, -20.0, 0.0, 20.0, 90.0, 104.0])
    raw_sc = torch.tensor([-100.0, -20.0, 0.0, 20.0, 88.0])
    u = torch.tensor([0.5, -0.5, 0.5, 0.5])
    quats = torch.stack([torch.zeros(4), 1e-13 * u, 5e-13 * u, 2e-12 * u, torch.tensor([0.0, 1e-20, 0.0, 0.0])])
    E = 7                                                   # rows that hold an edge value
    with torch.no_grad():
        pc0._rotation.copy_(sc["rotations"].to(DEV))
        pc0._opacity[:7, 0] = raw_op.to(DEV)
        pc0._scaling[:5] = raw_sc.to(DEV)[:, None].expand(5, 3)
        pc0._scaling[5] = torch.tensor([88.0, -100.0, 0.0], device=DEV)     # the extremes side by side in one row
        pc0._rotation[:5] = quats.to(DEV)
        for a, b in zip(pc0.leaves(), pc1.leaves()):
            b.copy_(a)
    want = [pc0.get_xyz, pc0.get_features, pc0.get_opacity, pc0.get_scaling, pc0.get_rotation]
    got = list(pc1.activated())
    cots = [(2.0 * torch.rand(w.shape, generator=g) - 1.0).to(DEV) for w in want]      # |cotangent| <= 1: exp(88) * it stays finite
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.allclose(a, b, rtol=2e-6, atol=1e-7), (a - b).abs().max()
        assert not (torch.isnan(a) & torch.isfinite(b)).any()
    assert torch.isfinite(want[3]).all() and want[3].max().item() > 1e38 and want[2][0].item() == 0.0 and want[2][6].item() == 1.0
    torch.autograd.backward(want[1:], cots[1:])
    torch.autograd.backward(got[1:], cots[1:])
    for a, b in zip(pc1.leaves()[1:], pc0.leaves()[1:]):
        assert a.grad is not None and not (torch.isnan(a.grad) & torch.isfinite(b.grad)).any()
        assert torch.isfinite(b.grad).all()
        big = b.grad.abs().max().item()
        assert torch.allclose(a.grad, b.grad, rtol=1e-4, atol=1e-5 * big), (a.grad - b.grad).abs().max()
        assert torch.allclose(a.grad[E:], b.grad[E:], rtol=1e-4, atol=1e-5), (a.grad[E:] - b.grad[E:]).abs().max()
    rg = pc0._rotation.grad
    assert rg[:3].abs().max().item() > 1e11 and rg[4].abs().max().item() > 1e11            # clamped denominator: g / 1e-12
