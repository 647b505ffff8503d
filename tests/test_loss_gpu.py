"""Fused photometric loss (csrc/loss.hip behind bags_loss_forward / bags_loss_backward) against the oracle, the reference's
golden vectors and, at the bench size, the separable PyTorch implementation."""
import functools
import os

import numpy as np
import pytest
import torch

import loss_cases as LC
from bags_raster import loss as L
from oracle import loss_oracle as LO

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _fused(a, b, g_l1, g_ssim):
    at = torch.from_numpy(a).to(DEV).requires_grad_(True)
    bt = torch.from_numpy(b).to(DEV)
    l1, s = L.fused_l1_ssim(at, bt)
    (g_l1 * l1 + g_ssim * s).backward()
    return l1.item(), s.item(), at.grad.cpu().numpy()


def test_fused_loss_matches_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "loss.npz"))
    l1, s, grad = _fused(g["a"], g["b"], 0.8, -0.2)
    assert abs(l1 - float(g["l1"])) < 1e-6 and abs(s - float(g["ssim"])) < 1e-5
    np.testing.assert_allclose(grad, g["dloss_da"], rtol=1e-3, atol=2e-8)
    at = torch.from_numpy(g["a"]).to(DEV); bt = torch.from_numpy(g["b"]).to(DEV)
    assert abs(L.fused_photometric_loss(at, bt).item() - float(g["loss"])) < 1e-5
    g = np.load(os.path.join(golden_dir, "loss_odd.npz"))
    l1, s, g1 = _fused(g["a"], g["b"], 1.0, 0.0)
    _, _, g2 = _fused(g["a"], g["b"], 0.0, 1.0)
    assert abs(l1 - float(g["l1"])) < 1e-6 and abs(s - float(g["ssim"])) < 1e-5
    np.testing.assert_allclose(g1, g["dl1_da"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(g2, g["dssim_da"], rtol=2e-3, atol=3e-8)


@pytest.mark.parametrize("shape", [(3, 64, 96), (1, 5, 7), (3, 33, 31), (4, 100, 17), (3, 1, 1)])
def test_fused_loss_matches_oracle(shape):
    rng = np.random.default_rng(sum(shape))
    a = rng.random(shape, dtype=np.float32)
    b = np.clip(a + 0.2 * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    b[..., : shape[2] // 2] = a[..., : shape[2] // 2]          # identical region: SSIM == 1, sign(0) == 0 there
    l1o, so, go = LO.loss_and_grad(a, b, 0.8, -0.2)
    l1, s, grad = _fused(a, b, 0.8, -0.2)
    assert abs(l1 - l1o) < 1e-6 and abs(s - so) < 2e-5
    scale = np.abs(go).max()
    assert np.abs(grad - go).max() <= 2e-4 * scale + 1e-9, np.abs(grad - go).max() / scale


def test_fused_loss_full_size_properties():
    """1080p: agrees with the separable PyTorch implementation, is bitwise reproducible, SSIM(x, x) == 1 with zero
    gradient, and the gradient is linear in the upstream scalars."""
    g = torch.Generator().manual_seed(5)
    a = torch.rand(3, 1080, 1920, generator=g).to(DEV)
    b = (a + 0.1 * torch.randn(3, 1080, 1920, generator=g).to(DEV)).clamp(0, 1)
    a1 = a.clone().requires_grad_(True); a2 = a.clone().requires_grad_(True)
    lf = L.fused_photometric_loss(a1, b); lf.backward()
    lt = L.photometric_loss(a2, b); lt.backward()
    assert abs(lf.item() - lt.item()) < 1e-5
    rel = (a1.grad - a2.grad).norm() / a2.grad.norm()
    assert rel.item() < 1e-4, rel.item()
    a3 = a.clone().requires_grad_(True)
    lf2 = L.fused_photometric_loss(a3, b); lf2.backward()
    assert torch.equal(lf, lf2) and torch.equal(a1.grad, a3.grad)
    a4 = a.clone().requires_grad_(True)
    l1, s = L.fused_l1_ssim(a4, a)
    assert l1.item() == 0.0 and abs(s.item() - 1.0) < 1e-6
    (3.0 * s).backward()
    assert a4.grad.abs().max().item() < 1e-9
    a5 = a.clone().requires_grad_(True)
    l1, s = L.fused_l1_ssim(a5, b); (2.0 * (0.8 * l1 - 0.2 * s)).backward()
    assert ((a5.grad - 2.0 * a1.grad).norm() / a1.grad.norm()).item() < 1e-6


@pytest.mark.parametrize("lam", [0.2, 0.0, 1.0, 0.37])
def test_combined_loss_equals_the_two_term_composition(lam):
    """bags_photometric_loss_* (the combination of train.py:325 inside the kernels) against the same expression written in
    PyTorch on the two terms: the loss to two ulp, dL/dimage to rounding, scaled upstream gradients,
    and the two logging terms detached."""
    g = torch.Generator().manual_seed(11)
    a = torch.rand(3, 70, 93, generator=g).to(DEV)
    b = (a + 0.1 * torch.randn(3, 70, 93, generator=g).to(DEV)).clamp(0, 1)
    a1 = a.clone().requires_grad_(True); a2 = a.clone().requires_grad_(True)
    loss, l1c, sc = L.fused_photometric_loss(a1, b, lam, return_terms=True)
    l1, s = L.fused_l1_ssim(a2, b)
    ref = (1.0 - lam) * l1 + lam * (1.0 - s)
    assert abs(loss.item() - ref.item()) <= 2.5e-7 and torch.equal(l1c, l1) and torch.equal(sc, s)     # (1 - lambda is rounded once on each side)
    assert not l1c.requires_grad and not sc.requires_grad and loss.requires_grad
    (2.5 * loss).backward(); (2.5 * ref).backward()
    scale = a2.grad.abs().max().item()
    assert (a1.grad - a2.grad).abs().max().item() <= 1e-6 * scale + 1e-12
    with pytest.raises(RuntimeError, match="lambda_dssim"):
        L.fused_photometric_loss(a1, b, 1.5)


def test_fused_loss_rejects_bad_arguments():
    a = torch.rand(3, 8, 8)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        L.fused_l1_ssim(a, a)
    with pytest.raises(RuntimeError, match="float32"):
        L.fused_l1_ssim(a.to(DEV).double(), a.to(DEV).double())
    with pytest.raises(RuntimeError, match="one shape"):
        L.fused_l1_ssim(a.to(DEV), torch.rand(3, 8, 9, device=DEV))


# ------------------------------------------------------------------------------------------------ untested paths
@functools.lru_cache(maxsize=None)
def _case(kind, shape):
    a, b = LC.make_pair(kind, shape)
    ref = LC.reference(a, b)
    ref["grad"].setflags(write=False)                  # shared among the tests: read only
    return a, b, ref


@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("shape", LC.RAGGED_SHAPES)
def test_fused_loss_vector_path_at_ragged_widths(shape, kind):
    """W % 4 == 0 and W % 32 != 0: the forward stages 16-byte groups and the last tile column is partly outside the image.
    Noise, flat bright (0.9 +- 1e-3: E[a^2] - mu^2 cancels against C2), dark (< 1e-3), out of range ([-1, 2)) and a 7x5
    checkerboard against the float64 oracle, upstream scalars (0.8, -0.2).

    The bar is measured on the CPU from the reference alone (tests/loss_cases.py): err32 is what the float32 PyTorch loss
    loses against the oracle on the same input, and the kernel may lose 4 * err32 + floor (gradient floor 1e-6 max|grad|,
    L1 2e-7, SSIM 5e-7) -- both round the same 11+11-term sums in float32, in another order.  Largest gradient error / err32
    measured on the MI355X: noise 0.84, flat bright 1.65, dark 1.27, out of range 1.62, checkerboard 1.09.  (What the bar
    cannot see: the outermost window taps weigh 1.0e-3, so one of them wrong by 1e-4 moves the gradient by 1e-7 of its
    maximum, which is below err32 itself; the same relative error on the centre tap fails 19 of these 25 cases.)"""
    a, b, ref = _case(kind, shape)
    at = torch.from_numpy(a).to(DEV).requires_grad_(True)
    bt = torch.from_numpy(b).to(DEV)
    assert shape[2] % 4 == 0 and shape[2] % 32 != 0 and at.data_ptr() % 16 == 0 and bt.data_ptr() % 16 == 0
    l1, s, grad = _fused(a, b, LC.G_L1, LC.G_SSIM)
    bar_g, bar_l1, bar_s = LC.bars(ref)
    err = np.abs(grad.astype(np.float64) - ref["grad"])
    c, y, x = np.unravel_index(err.argmax(), err.shape)
    e_g, e_l1, e_s = float(err.max()), abs(l1 - ref["l1"]), abs(s - ref["ssim"])
    print(f"{kind} {shape}: grad err {e_g:.3e} at (c,y,x)=({c},{y},{x}) bar {bar_g:.3e} err32 {ref['err32_grad']:.3e} "
          f"ratio {e_g / max(ref['err32_grad'], 1e-300):.2f} | l1 {e_l1:.2e}/{bar_l1:.2e} | ssim {e_s:.2e}/{bar_s:.2e} "
          f"(err32 {ref['err32_ssim']:.2e})")
    assert np.isfinite(grad).all()
    assert e_l1 <= bar_l1, (e_l1, bar_l1)
    assert e_s <= bar_s, (e_s, bar_s, ref["err32_ssim"])
    assert e_g <= bar_g, (e_g, bar_g, ref["err32_grad"], (c, y, x))


def _offset_copy(t):
    """The same values at a 4-byte storage offset: contiguous, but not 16-byte aligned (the scalar staging branch)."""
    buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("shape", [(3, 40, 44), (3, 64, 96)])
def test_fused_loss_vector_and_scalar_staging_give_the_same_bits(shape):
    """The two staging branches of loss_fwd_kernel put the same numbers into LDS and share everything after it: an image, a
    target or both at a misaligned base (scalar branch at a width that could have taken the vector one) give the same two
    scalars and the same gradient bit for bit."""
    a, b = LC.make_pair("noise", shape)
    a0, b0 = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    assert a0.data_ptr() % 16 == 0 and b0.data_ptr() % 16 == 0

    def run(at, bt):
        at = at.requires_grad_(True)
        l1, s = L.fused_l1_ssim(at, bt)
        (LC.G_L1 * l1 + LC.G_SSIM * s).backward()
        return l1.detach(), s.detach(), at.grad
    want = run(a0.clone(), b0)
    for off_a, off_b in ((True, False), (False, True), (True, True)):
        at = _offset_copy(a0) if off_a else a0.clone()
        bt = _offset_copy(b0) if off_b else b0
        assert (at.data_ptr() % 16 != 0) == off_a and (bt.data_ptr() % 16 != 0) == off_b
        got = run(at, bt)
        for g, w, name in zip(got, want, ("l1", "ssim", "grad")):
            assert torch.equal(g, w), (off_a, off_b, name, (g - w).abs().max().item())


def test_fused_loss_one_sided_backward():
    """backward() through one of the two scalars only: d l1 / d image is exactly float32(1/n) * sign(a - b) (zero where
    a == b), and d ssim / d image is the (0, 1) combination bit for bit."""
    shape = (3, 40, 44)
    a, b, _ = _case("noise", shape)
    at = torch.from_numpy(a).to(DEV).requires_grad_(True); bt = torch.from_numpy(b).to(DEV)
    l1, _ = L.fused_l1_ssim(at, bt)
    l1.backward()
    want = torch.sign(at.detach() - bt) * float(np.float32(1.0 / a.size))
    assert (at.detach() == bt).any() and torch.equal(at.grad, want)
    assert (at.grad[at.detach() == bt] == 0).all()
    a2 = torch.from_numpy(a).to(DEV).requires_grad_(True)
    _, s = L.fused_l1_ssim(a2, bt)
    s.backward()
    _, _, g01 = _fused(a, b, 0.0, 1.0)
    assert np.array_equal(a2.grad.cpu().numpy(), g01) and np.abs(g01).max() > 0


@pytest.mark.parametrize("lam", [0.2, 0.0, 1.0, 0.37])
@pytest.mark.parametrize("shape", [(3, 70, 93), (3, 40, 44)])
def test_combined_loss_equals_the_two_term_composition_by_shape(shape, lam):
    """test_combined_loss_equals_the_two_term_composition at a scalar-staged (W = 93) and a vector-ragged (W = 44) shape."""
    g = torch.Generator().manual_seed(11)
    a = torch.rand(*shape, generator=g).to(DEV)
    b = (a + 0.1 * torch.randn(*shape, generator=g).to(DEV)).clamp(0, 1)
    a1 = a.clone().requires_grad_(True); a2 = a.clone().requires_grad_(True)
    loss, l1c, sc = L.fused_photometric_loss(a1, b, lam, return_terms=True)
    l1, s = L.fused_l1_ssim(a2, b)
    ref = (1.0 - lam) * l1 + lam * (1.0 - s)
    assert abs(loss.item() - ref.item()) <= 2.5e-7 and torch.equal(l1c, l1) and torch.equal(sc, s)
    assert not l1c.requires_grad and not sc.requires_grad and loss.requires_grad
    (2.5 * loss).backward(); (2.5 * ref).backward()
    scale = a2.grad.abs().max().item()
    assert (a1.grad - a2.grad).abs().max().item() <= 1e-6 * scale + 1e-12
