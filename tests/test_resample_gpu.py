"""Fused distortion resampling (csrc/resample.hip behind bags_resample_forward / bags_resample_backward) against the reference's
golden vectors, the numpy oracle and, at full size, the PyTorch pipeline the reference runs."""
import os

import numpy as np
import pytest
import torch

from bags_raster.distortion import resample_image, resample_image_torch
from oracle import resample_oracle as RO

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _hip(image, ctrl, fhw, chw, cot):
    img = torch.from_numpy(image).to(DEV).requires_grad_(True)
    ctl = torch.from_numpy(ctrl).to(DEV).requires_grad_(True)
    out, mask = resample_image(img, ctl, fhw, chw)
    (out * torch.from_numpy(cot).to(DEV)).sum().backward()
    return out.detach().cpu().numpy(), mask.cpu().numpy(), img.grad.cpu().numpy(), ctl.grad.cpu().numpy()


def test_resample_matches_reference_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "resample.npz"))
    fhw, chw = tuple(int(v) for v in g["flow_hw"]), tuple(int(v) for v in g["crop_hw"])
    out, mask, gi, gc = _hip(g["image"], g["ctrl"], fhw, chw, g["cot"])
    np.testing.assert_allclose(out, g["out"], atol=2e-4)               # the reference's crop is a second grid_sample (1e-4 px)
    assert (mask != g["mask"]).mean() < 0.002
    np.testing.assert_allclose(gi, g["d_image"], atol=3e-4)
    np.testing.assert_allclose(gc, g["d_ctrl"], rtol=2e-3, atol=2e-3 * np.abs(g["d_ctrl"]).max())


@pytest.mark.parametrize("C,H,W,h,w,fhw,chw", [(3, 33, 47, 5, 6, (40, 52), (31, 45)), (1, 8, 8, 2, 2, (9, 9), (9, 9)),
                                               (3, 20, 30, 20, 30, (20, 30), (20, 30)), (4, 17, 5, 3, 7, (64, 64), (1, 1))])
def test_resample_matches_oracle(C, H, W, h, w, fhw, chw):
    rng = np.random.default_rng(C * 100 + H)
    image = rng.random((C, H, W), dtype=np.float32)
    gy, gx = np.meshgrid(np.linspace(-1.3, 1.3, h), np.linspace(-1.3, 1.3, w), indexing="ij")   # reaches outside: zero padding
    ctrl = (np.stack((gx, gy), -1) + 0.1 * rng.standard_normal((h, w, 2))).astype(np.float32)
    cot = rng.standard_normal((C,) + chw).astype(np.float32)
    out, mask, gi, gc = _hip(image, ctrl, fhw, chw, cot)
    o_w, m_w = RO.forward(image, ctrl, fhw, chw)
    gi_w, gc_w = RO.backward(image, ctrl, fhw, chw, cot)
    np.testing.assert_allclose(out, o_w, atol=5e-5)                    # fp32 sampling positions: ~1e-5 px
    assert (mask != m_w).mean() < 0.01
    np.testing.assert_allclose(gi, gi_w, atol=2e-4 * max(1.0, np.abs(gi_w).max()))
    np.testing.assert_allclose(gc, gc_w, atol=2e-3 * max(1e-6, np.abs(gc_w).max()))


def test_resample_full_size_against_pytorch_pipeline():
    """Rendered 1080p image, 68x120 control flow upsampled to 1188x2112, cropped to 1080x1920 (the shape of the reference's
    flow_scale = 1.1 setting): agrees with interpolate + grid_sample + center_crop on the GPU, forward and backward."""
    g = torch.Generator().manual_seed(3)
    H, W, h, w, fhw, chw = 1080, 1920, 68, 120, (1188, 2112), (1080, 1920)
    image = torch.rand(3, H, W, generator=g).to(DEV)
    gy, gx = torch.meshgrid(torch.linspace(-1.1, 1.1, h), torch.linspace(-1.1, 1.1, w), indexing="ij")
    ctrl = (torch.stack((gx, gy), -1) + 0.01 * torch.randn(h, w, 2, generator=g)).to(DEV)
    cot = torch.randn(3, *chw, generator=g).to(DEV)
    def run(fn, dt):
        img = image.to(dt).clone().requires_grad_(True); ctl = ctrl.to(dt).clone().requires_grad_(True)
        out, mask = fn(img, ctl, fhw, chw)
        (out * cot.to(dt)).sum().backward()
        return out.detach().double(), mask.double(), img.grad.double(), ctl.grad.double()
    hip, t32, t64 = run(resample_image, torch.float32), run(resample_image_torch, torch.float32), run(resample_image_torch, torch.float64)
    d = (hip[0] - t64[0]).abs()                                        # fp32 sampling positions near x = 1900: ~1e-4 px,
    assert d.max().item() < 1e-3 and d.mean().item() < 5e-5            # times the O(1)/px slope of a noise image
    assert d.max().item() <= 1.5 * (t32[0] - t64[0]).abs().max().item() + 1e-5
    # the mask is an exact == 0 test: pixels on the rim of the zero-padding region flip with the last bit of the position
    mm = lambda a: (a[1] != t64[1]).double().mean().item()
    assert mm(hip) <= 1.5 * mm(t32) + 1e-4 and mm(hip) < 5e-3, (mm(hip), mm(t32))
    # The float32 PyTorch pipeline is itself ~5e-3 away from float64 in dL/dflow on a noise image (its crop is a second
    # grid_sample whose integer grid is reproduced to 1e-4 px); the fused kernels must be at least as close to float64.
    rel = lambda a, b: ((a - b).norm() / b.norm()).item()
    for k in (2, 3):
        assert rel(hip[k], t64[k]) <= 1.5 * rel(t32[k], t64[k]) + 1e-4, (k, rel(hip[k], t64[k]), rel(t32[k], t64[k]))
    print("dL/dimage rel err vs float64: fused %.2e, pytorch32 %.2e; dL/dflow: fused %.2e, pytorch32 %.2e" %
          (rel(hip[2], t64[2]), rel(t32[2], t64[2]), rel(hip[3], t64[3]), rel(t32[3], t64[3])))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn, name in ((resample_image, "fused"), (resample_image_torch, "pytorch")):
        img = image.clone().requires_grad_(True); ctl = ctrl.clone().requires_grad_(True)
        fn(img, ctl, fhw, chw)[0].backward(cot); torch.cuda.synchronize()
        e0.record()
        for _ in range(10):
            img.grad = None; ctl.grad = None
            fn(img, ctl, fhw, chw)[0].backward(cot)
        e1.record(); torch.cuda.synchronize()
        print(f"resample fwd+bwd @1080p {name}: {e0.elapsed_time(e1) / 10:.3f} ms")


def test_resample_backward_is_bitwise_reproducible_and_handles_minification():
    """dL/dimage is accumulated per source tile in 64-bit fixed point (no global atomics): two runs must agree bit for bit.
    The second flow squeezes the whole 160x208 output into the centre of the image, so that far more than 32 output tiles
    sample one source tile: the per-tile lists overflow and the gather falls back to testing every output tile's box."""
    rng = np.random.default_rng(11)
    C, H, W, h, w, fhw, chw = 3, 96, 128, 6, 8, (176, 224), (160, 208)
    image = rng.random((C, H, W), dtype=np.float32)
    cot = rng.standard_normal((C,) + chw).astype(np.float32)
    for span in (1.05, 0.08):
        gy, gx = np.meshgrid(np.linspace(-span, span, h), np.linspace(-span, span, w), indexing="ij")
        ctrl = (np.stack((gx, gy), -1) + 0.02 * span * rng.standard_normal((h, w, 2))).astype(np.float32)
        a = _hip(image, ctrl, fhw, chw, cot)
        b = _hip(image, ctrl, fhw, chw, cot)
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        gi_w, gc_w = RO.backward(image, ctrl, fhw, chw, cot)
        np.testing.assert_allclose(a[2], gi_w, atol=2e-4 * max(1.0, np.abs(gi_w).max()))
        np.testing.assert_allclose(a[3], gc_w, atol=2e-3 * max(1e-6, np.abs(gc_w).max()))
        if span < 0.5:
            assert (np.abs(gi_w).reshape(C, -1).sum(0) > 0).mean() < 0.05      # everything lands in a small patch of the image


def test_resample_rejects_bad_arguments():
    with pytest.raises(RuntimeError, match="GPU tensor"):
        resample_image(torch.rand(3, 8, 8), torch.rand(2, 2, 2), (8, 8), (8, 8))
    with pytest.raises(RuntimeError, match="exceeds"):
        resample_image(torch.rand(3, 8, 8, device=DEV), torch.rand(2, 2, 2, device=DEV), (8, 8), (9, 8))


# ------------------------------------------------------------------------------------------------ untested paths
GEOM = (33, 47, 5, 6, (40, 52), (31, 45))                    # H, W, h, w, flow, crop of the first oracle case
MINI = (96, 128, 6, 8, (176, 224), (160, 208))               # geometry of the minification test


def _inputs(C, H, W, h, w, chw, seed, span=1.3, jitter=0.1):
    """Image, control flow and cotangent as test_resample_matches_oracle makes them.  An axis with a single control node has no
    extent to span: its coordinate is 0.2 (inside the image), so that the samples do not all land in the zero padding."""
    rng = np.random.default_rng(seed)
    image = rng.random((C, H, W), dtype=np.float32)
    axis = lambda n: np.linspace(-span, span, n) if n > 1 else np.array([0.2])
    gy, gx = np.meshgrid(axis(h), axis(w), indexing="ij")
    ctrl = (np.stack((gx, gy), -1) + jitter * rng.standard_normal((h, w, 2))).astype(np.float32)
    cot = rng.standard_normal((C,) + tuple(chw)).astype(np.float32)
    return image, ctrl, cot


def _check_against_oracle(inputs, fhw, chw):
    """The bars of test_resample_matches_oracle."""
    image, ctrl, cot = inputs
    out, mask, gi, gc = _hip(image, ctrl, fhw, chw, cot)
    o_w, m_w = RO.forward(image, ctrl, fhw, chw)
    gi_w, gc_w = RO.backward(image, ctrl, fhw, chw, cot)
    assert np.abs(o_w).max() > 0.1 and np.abs(gi_w).max() > 0.1 and np.abs(gc_w).max() > 0.1      # not all in the zero padding
    np.testing.assert_allclose(out, o_w, atol=5e-5)
    assert (mask != m_w).mean() < 0.01
    np.testing.assert_allclose(gi, gi_w, atol=2e-4 * max(1.0, np.abs(gi_w).max()))
    np.testing.assert_allclose(gc, gc_w, atol=2e-3 * max(1e-6, np.abs(gc_w).max()))
    return gi, gc, gi_w, gc_w


@pytest.mark.parametrize("C", [5, 7, 24])
def test_resample_more_than_four_channels(C):
    """C > 4: listed tiles take the serial accumulation loop of resample_gather_kernel (cotangents in go[24]) instead of the
    batched one; 24 channels fill the 48 KB fixed-point accumulator."""
    H, W, h, w, fhw, chw = GEOM
    _check_against_oracle(_inputs(C, H, W, h, w, chw, seed=C * 100 + H), fhw, chw)


def test_resample_five_channels_through_the_overflow_fallback():
    """The minification flow (span 0.08) of test_resample_backward_is_bitwise_reproducible_and_handles_minification at C = 5:
    the per-tile lists overflow, so the serial loop runs over every output tile's box with more than four channels."""
    H, W, h, w, fhw, chw = MINI
    image, ctrl, cot = _inputs(5, H, W, h, w, chw, seed=11, span=0.08, jitter=0.02 * 0.08)
    gi, _, gi_w, _ = _check_against_oracle((image, ctrl, cot), fhw, chw)
    assert (np.abs(gi_w).reshape(5, -1).sum(0) > 0).mean() < 0.05      # everything lands in a small patch: far over 32 tiles per list
    assert np.array_equal(gi, _hip(image, ctrl, fhw, chw, cot)[2])


def test_resample_rejects_more_than_24_channels():
    with pytest.raises(RuntimeError, match="at most 24 channels"):
        resample_image(torch.rand(25, 8, 8, device=DEV), torch.rand(2, 2, 2, device=DEV), (8, 8), (8, 8))


@pytest.mark.parametrize("C", [3, 5])
def test_resample_one_gradient_at_a_time(C):
    """Only the image, or only the flow, requires grad (the bbox == NULL / gflow == NULL halves of resample_bwd_pixels_kernel):
    each gradient is computed from intermediates the other does not touch, so it equals the both-gradients run bit for bit."""
    H, W, h, w, fhw, chw = GEOM
    image, ctrl, cot = _inputs(C, H, W, h, w, chw, seed=C * 100 + H)
    cot_t = torch.from_numpy(cot).to(DEV)

    def run(need_img, need_ctl):
        img = torch.from_numpy(image).to(DEV).requires_grad_(need_img)
        ctl = torch.from_numpy(ctrl).to(DEV).requires_grad_(need_ctl)
        out, _ = resample_image(img, ctl, fhw, chw)
        out.backward(cot_t)
        return img.grad, ctl.grad
    gi, gc = run(True, True)
    assert gi.abs().max().item() > 0.1 and gc.abs().max().item() > 0.1
    gi1, gc1 = run(True, False)
    assert gc1 is None and torch.equal(gi1, gi)
    gi2, gc2 = run(False, True)
    assert gi2 is None and torch.equal(gc2, gc)


@pytest.mark.parametrize("h,w,fhw,chw", [(1, 6, (40, 52), (31, 45)), (5, 1, (40, 52), (31, 45)), (1, 1, (40, 52), (31, 45)),
                                         (20, 30, (12, 18), (10, 16)), (5, 6, (41, 53), (32, 46))])
def test_resample_control_grid_shapes(h, w, fhw, chw):
    """One row, one column and one node of control flow (first and last node coincide), a control grid finer than the flow
    (less than one destination pixel per control cell) and an odd crop margin ((41 - 32) / 2 rounds down)."""
    H, W = GEOM[:2]
    _, gc, _, gc_w = _check_against_oracle(_inputs(3, H, W, h, w, chw, seed=h * 100 + w), fhw, chw)
    assert gc.shape == (h, w, 2)
    if h > fhw[0]:                                                     # the finer grid has nodes that no flow pixel interpolates from
        assert (np.abs(gc_w).sum(-1) == 0).any()


def test_resample_flow_out():
    """bags_resample_forward's flow_out (the interpolated flow at the cropped pixels, which resample_image never asks for):
    against the oracle's flow to float32 rounding of a four-term sum of values up to ~1.3; asking for it changes nothing else."""
    from bags_raster import _lib as BL
    H, W, h, w, fhw, chw = GEOM
    image, ctrl, _ = _inputs(3, H, W, h, w, chw, seed=300 + H)
    img, ctl = torch.from_numpy(image).to(DEV), torch.from_numpy(ctrl).to(DEV)
    lib = BL.load()

    def run(with_flow):
        out = torch.full((3,) + chw, float("nan"), device=DEV); mask = torch.full((1,) + chw, float("nan"), device=DEV)
        flow = torch.full(chw + (2,), float("nan"), device=DEV) if with_flow else None
        BL.check(lib.bags_resample_forward(img.data_ptr(), 3, H, W, ctl.data_ptr(), h, w, fhw[0], fhw[1], chw[0], chw[1], out.data_ptr(),
                                           mask.data_ptr(), flow.data_ptr() if with_flow else None,
                                           torch.cuda.current_stream().cuda_stream), "bags_resample_forward")
        torch.cuda.synchronize()
        return out, mask, flow
    out0, mask0, _ = run(False)
    out1, mask1, flow = run(True)
    assert torch.equal(out0, out1) and torch.equal(mask0, mask1) and not torch.isnan(out0).any()
    want = RO.interpolated_flow(ctrl, fhw, chw)
    err = np.abs(flow.cpu().numpy().astype(np.float64) - want)
    assert np.abs(want).max() > 1.0 and (err <= 2e-6 * (1 + np.abs(want))).all(), err.max()
    o2, m2 = resample_image(img, ctl, fhw, chw)
    assert torch.equal(o2, out0) and torch.equal(m2, mask0)


def _hip_cot(image, ctrl, fhw, chw, cot):
    """_hip with the cotangent handed to backward() as it is (no multiplication by ones in between)."""
    img = torch.from_numpy(image).to(DEV).requires_grad_(True)
    ctl = torch.from_numpy(ctrl).to(DEV).requires_grad_(True)
    out, mask = resample_image(img, ctl, fhw, chw)
    out.backward(torch.from_numpy(np.ascontiguousarray(cot)).to(DEV))
    return out.detach().cpu().numpy(), mask.cpu().numpy(), img.grad.cpu().numpy(), ctl.grad.cpu().numpy()


def test_resample_fixed_point_scaling():
    """The quantum of the fixed-point accumulator follows the largest cotangent by powers of two: scaling the cotangent by
    2^40 or 2^-40 scales both gradients by exactly that (every step is a power-of-two shift of the same integers; a cotangent
    of order 1 keeps every product normal).  A zero cotangent gives exact zeros, a one-hot cotangent the four taps of that
    pixel, and a cotangent of 1e-36 (below the 2^-100 clamp of the scale) stays finite and rounds towards zero."""
    C = 3
    H, W, h, w, fhw, chw = GEOM
    image, ctrl, cot = _inputs(C, H, W, h, w, chw, seed=C * 100 + H)
    cot = np.where(np.abs(cot) < 1e-3, np.float32(1e-3), cot).astype(np.float32)
    _, _, gi, gc = _hip_cot(image, ctrl, fhw, chw, cot)
    assert np.abs(gi).max() > 0.1 and np.abs(gc).max() > 0.1
    for k in (40, -40):
        _, _, gi_k, gc_k = _hip_cot(image, ctrl, fhw, chw, np.ldexp(cot, k))
        assert np.array_equal(gi_k, np.ldexp(gi, k)) and np.array_equal(gc_k, np.ldexp(gc, k)), k
    _, _, gi_0, gc_0 = _hip_cot(image, ctrl, fhw, chw, np.zeros_like(cot))
    assert not gi_0.any() and not gc_0.any()
    # one output pixel whose four taps are all inside the image, and one on the rim of the zero padding
    p = RO._prepare(image, ctrl, fhw, chw)
    inside = lambda dy, dx: (p["y0"] + dy >= 0) & (p["y0"] + dy < H) & (p["x0"] + dx >= 0) & (p["x0"] + dx < W)
    wsum = sum(np.where(inside(dy, dx), (p["fy"] if dy else 1 - p["fy"]) * (p["fx"] if dx else 1 - p["fx"]), 0.0)
               for dy in (0, 1) for dx in (0, 1))
    n_in = sum(inside(dy, dx).astype(int) for dy in (0, 1) for dx in (0, 1))
    # all four taps inside: the weights sum to 1 whatever the position.  On the rim the sum depends on the float32 sampling
    # position, which flow_out's bar (2e-6 * (1 + |flow|), |flow| < 1.6) puts within 2.6e-6 * (W - 1) / 2 px of the oracle's.
    picks = [(np.argwhere(n_in == 4)[0], 1.5, 1e-6), (np.argwhere(n_in == 4)[-1], -0.75, 1e-6),
             (np.argwhere((n_in > 0) & (n_in < 4) & (wsum > 0.05) & (wsum < 0.95))[0], 2.0, None)]
    for (y, x), value, rel in picks:
        hot = np.zeros_like(cot); hot[:, y, x] = value
        _, _, gi_h, _ = _hip_cot(image, ctrl, fhw, chw, hot)
        want = value * wsum[y, x]
        tol = rel * abs(want) if rel else abs(value) * 2.6e-6 * 0.5 * ((W - 1) + (H - 1)) + 1e-6 * abs(want)
        for ch in range(C):
            assert 1 <= np.count_nonzero(gi_h[ch]) <= 4
            assert abs(gi_h[ch].astype(np.float64).sum() - want) <= tol, (y, x, ch, gi_h[ch].sum(), want)
    tiny = (cot * np.float32(1e-36) / np.abs(cot).max()).astype(np.float32)
    _, _, gi_t, gc_t = _hip_cot(image, ctrl, fhw, chw, tiny)
    gi_w, gc_w = RO.backward(image, ctrl, fhw, chw, tiny)
    assert np.isfinite(gi_t).all() and np.isfinite(gc_t).all()
    assert np.abs(gi_t - gi_w).max() < 1e-30 and np.abs(gc_t - gc_w).max() < 1e-30
