"""The fused lens network (csrc/lens_field.hip) on the MI355X: against the float64 reference under the measured bar of
tests/lens_cases.py, the bitwise properties (row independence, shape independence, run-to-run, stream, optional gradients,
M = 0), and the chain into resample_image."""
import ctypes as C

import pytest
import torch

import lens_cases as LC
from bags_raster import LensField, _lib as L, lens_field
from bags_raster.distortion import resample_image
from bags_raster.lens_field import lens_field_inverse, param_count

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _fused(name, want_x=True, want_p=True):
    c = LC.make_case(name)
    p = c["params"].to(DEV).requires_grad_(want_p)
    x = c["x"].to(DEV).requires_grad_(want_x)
    y = lens_field(p, x, *LC.dims(name))
    y.backward(c["cot"].to(DEV))
    return y.detach(), x.grad, p.grad


def _c_backward(name, x, cot, want_x, want_p, fill=float("nan")):
    """bags_lens_field_backward itself, with real NULLs for the gradients that are not asked for."""
    c = LC.make_case(name)
    B, H, n = LC.dims(name)
    p = c["params"].to(DEV)
    x, cot = x.to(DEV).reshape(-1, 2).contiguous(), cot.to(DEV).reshape(-1, 2).contiguous()
    M = x.shape[0]
    g_x = torch.full_like(x, fill) if want_x else None
    g_p = torch.full_like(p, fill) if want_p else None
    ws = torch.full((L.load().bags_lens_field_workspace_size(B, H, n, M),), 0xA5, dtype=torch.uint8, device=DEV)    # needs no zeroing
    L.call("bags_lens_field_backward", p.device, L.BagsLensField(B, H, n, 0, p.data_ptr()), x.data_ptr(), M, cot.data_ptr(), ws.data_ptr(),
           ws.numel(), L.ptr(g_x), L.ptr(g_p))
    return g_x, g_p


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_forward_and_gradients_match_the_float64_reference(name):
    """Forward by max-abs, grad_x and grad_params by relative L2, each at most 4 x what float32 PyTorch loses on this device on the
    same input, plus 16 float32 epsilons of the reference's scale."""
    got = _fused(name)
    assert got[0].shape == LC.CASES[name]["shape"] and got[1].shape == got[0].shape and got[2].shape == (param_count(*LC.dims(name)),)
    err, bars = LC.errors(name, got), LC.bars(name, DEV)
    print(name, "err", err, "bars", bars, "err32", LC.err32(name, DEV))
    assert all(e <= b for e, b in zip(err, bars)), (err, bars)


@pytest.mark.parametrize("name", LC.INVERTIBLE)
def test_inverse_matches_the_float64_inverse(name):
    c = LC.make_case(name)
    y = LC.inverse_input(name).to(DEV)
    x = lens_field_inverse(c["params"].to(DEV), y, *LC.dims(name), LC.INVERSE_ITERATIONS)
    assert x.shape == y.shape
    err, bar = float((x.double().cpu() - LC.inverse_reference(name)).abs().max()), LC.inverse_bar(name, DEV)
    print(name, "inverse err", err, "bar", bar)
    assert err <= bar, (err, bar)
    net = LensField(*LC.dims(name), device=DEV)
    with torch.no_grad():
        net.params.copy_(c["params"])
    assert torch.equal(net.inverse(y), x) and not net.inverse(y).requires_grad
    # zero iterations leave y, and the round trip comes back to the input
    assert torch.equal(net.inverse(y, 0), y)
    assert float((net.inverse(net(c["x"].to(DEV))) - c["x"].to(DEV)).abs().max()) < 1e-4


def test_a_row_does_not_depend_on_the_rows_around_it():
    """The tail and partition test: row i of forward(x) is forward(x[i:i+1])[0], bit for bit, for every row at M = 257."""
    name = "b3_h33_n2_m257"
    c = LC.make_case(name)
    p, x = c["params"].to(DEV), c["x"].to(DEV)
    with torch.no_grad():
        full = lens_field(p, x, *LC.dims(name))
        rows = torch.cat([lens_field(p, x[i:i + 1], *LC.dims(name)) for i in range(x.shape[0])])
        assert torch.equal(full, rows)
        # ... nor on where a slice starts
        assert torch.equal(lens_field(p, x[100:230], *LC.dims(name)), full[100:230])


def test_a_grid_is_its_flattened_form():
    name = "grid_b5_h64_n1"
    c = LC.make_case(name)
    y, gx, gp = _fused(name)
    assert y.shape == (68, 120, 2) and gx.shape == (68, 120, 2)
    p = c["params"].to(DEV).requires_grad_(True)
    x = c["x"].to(DEV).reshape(-1, 2).requires_grad_(True)
    yf = lens_field(p, x, *LC.dims(name))
    yf.backward(c["cot"].to(DEV).reshape(-1, 2))
    assert torch.equal(yf.detach(), y.reshape(-1, 2)) and torch.equal(x.grad, gx.reshape(-1, 2)) and torch.equal(p.grad, gp)
    # a non-contiguous view of the same points too
    xt = c["x"].to(DEV).permute(1, 0, 2)
    with torch.no_grad():
        assert torch.equal(lens_field(c["params"].to(DEV), xt, *LC.dims(name)), y.permute(1, 0, 2))


@pytest.mark.parametrize("name", ["b5_h64_n1_m1025", "strided_b2_h16_n1_m16449", "b3_h33_n2_m255"])
def test_backward_is_reproducible_on_any_stream(name):
    first = _fused(name)
    again = _fused(name)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = _fused(name)
    side.synchronize()
    torch.cuda.current_stream().wait_stream(side)
    assert all(torch.equal(a, b) for a, b in zip(first, other))


@pytest.mark.parametrize("name", ["b5_h64_n1_m1025", "b1_h64_n4_m1025", "b3_h33_n2_m257", "b1_h1_n0_m1", "strided_b2_h16_n1_m16449"])
def test_each_gradient_alone_is_the_pair(name):
    """Through the C entry with real NULLs: grad_x alone and grad_params alone are the bits of the pair (which are autograd's)."""
    c = LC.make_case(name)
    _, gx, gp = _fused(name)
    both = _c_backward(name, c["x"], c["cot"], True, True)
    assert torch.equal(both[0], gx) and torch.equal(both[1], gp)
    only_x = _c_backward(name, c["x"], c["cot"], True, False)
    only_p = _c_backward(name, c["x"], c["cot"], False, True)
    assert only_x[1] is None and only_p[0] is None
    assert torch.equal(only_x[0], gx) and torch.equal(only_p[1], gp)
    # autograd picks the same NULLs from needs_input_grad
    assert torch.equal(_fused(name, want_x=False)[2], gp) and _fused(name, want_x=False)[1] is None
    assert torch.equal(_fused(name, want_p=False)[1], gx) and _fused(name, want_p=False)[2] is None


def test_no_points():
    name = "b5_h64_n1_m1025"
    c = LC.make_case(name)
    p = c["params"].to(DEV).requires_grad_(True)
    for shape in ((0, 2), (0, 7, 2), (3, 0, 2)):
        x = torch.empty(shape, device=DEV, requires_grad=True)
        p.grad = None
        y = lens_field(p, x, *LC.dims(name))
        assert y.shape == shape
        y.sum().backward()
        assert p.grad.shape == p.shape and float(p.grad.abs().max()) == 0.0 and x.grad.shape == shape
    g_x, g_p = _c_backward(name, torch.empty(0, 2), torch.empty(0, 2), True, True)
    assert g_x.shape == (0, 2) and float(g_p.abs().max()) == 0.0                # zero-filled over the NaNs it held
    with torch.no_grad():
        assert lens_field_inverse(p, torch.empty(0, 2, device=DEV), *LC.dims(name)).shape == (0, 2)


def test_module_runs_fused_on_the_gpu_and_takes_other_dtypes():
    name = "b2_h16_n1_m65"
    c = LC.make_case(name)
    net = LensField(*LC.dims(name), device=DEV, seed=3)
    assert net.params.is_cuda
    with torch.no_grad():
        net.params.copy_(c["params"])
    x = c["x"].to(DEV)
    y = net(x)
    assert y.dtype == torch.float32 and y.grad_fn is not None and type(y.grad_fn).__name__.startswith("_LensField")
    assert torch.equal(y.detach(), _fused(name)[0])
    assert torch.equal(net(x.double()).detach(), y.detach())        # read as float32, like every wrapper here
    with pytest.raises(RuntimeError, match="AMD GPU"):
        net(c["x"])                                                 # a host tensor into the fused path: refused, not copied


def test_chain_into_resample_image():
    """flow = lens(control_points); resample_image(image, flow, ...).sum().backward(): params.grad is, bit for bit, what
    bags_lens_field_backward gives for the dL/dctrl_flow that resample_image's backward returned."""
    gen = torch.Generator().manual_seed(5)
    net = LensField(5, 64, 1, device=DEV, seed=9)
    net.lipschitz_correction(iterations=20, generator=torch.Generator().manual_seed(6))
    gy, gx = torch.meshgrid(torch.linspace(-1, 1, 8), torch.linspace(-1, 1, 12), indexing="ij")
    ctrl = torch.stack((gx, gy), 2).to(DEV)                          # (8, 12, 2) control points, constants
    image = torch.rand(3, 32, 48, generator=gen).to(DEV)
    flow = net(ctrl)
    flow.retain_grad()
    out, _mask = resample_image(image, flow, (32, 48), (32, 48))
    out.sum().backward()
    assert flow.grad is not None and float(flow.grad.abs().max()) > 0 and float(net.params.grad.abs().max()) > 0
    B, H, n = net.dims
    p = net.params.detach()
    g_p = torch.full_like(p, float("nan"))
    ws = L.workspace(L.load().bags_lens_field_workspace_size(B, H, n, 96), p.device)
    L.call("bags_lens_field_backward", p.device, L.BagsLensField(B, H, n, 0, p.data_ptr()), ctrl.data_ptr(), 96, flow.grad.data_ptr(), ws.data_ptr(),
           ws.numel(), None, g_p.data_ptr())
    assert torch.equal(net.params.grad, g_p)
