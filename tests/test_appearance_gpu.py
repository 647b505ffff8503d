"""GPU checks of the appearance step: bags_raster.apply_appearance / AppearanceBank (csrc/appearance.hip) against appearance_torch
in float64 on the cases of tests/appearance_cases.py, held to that module's bars; the bitwise properties of its two paths, its
optional outputs and its sums; and the chain resample_image -> AppearanceBank.apply -> fused_photometric_loss."""
import ctypes as C

import pytest
import torch

import appearance_cases as A
from bags_raster import AppearanceBank, _lib as L, appearance_torch, apply_appearance
from bags_raster.appearance import NEUTRAL, _ptr_field
from bags_raster.distortion import resample_image
from bags_raster.loss import fused_photometric_loss
from bags_raster.pose_bank import _row_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
VECTOR_SHAPES = tuple(s for s in A.SHAPES if s[1] % 4 == 0)          # (16, 64) and the strided shape


def _place(t, offset):
    """``t`` as a float32 GPU tensor: at the start of an allocation (16-byte aligned), or -- ``offset`` -- as a view 4 bytes into
    a larger one, which no float4 access may touch: the scalar path."""
    n = t.numel()
    buf = torch.empty(n + 4, dtype=F32, device=DEV)
    v = (buf[1:1 + n] if offset else buf[:n]).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 if offset else 0) and v.is_contiguous()
    return v


def _run(c, offset=False, stacked=False, views=None, scale=1.0):
    """Forward and backward through autograd: (out (V,3,H,W), dL/dimages (V,3,H,W), dL/dtable (N,16)) on the host."""
    idx = list(range(c["V"])) if views is None else list(views)
    rows = [c["rows"][i] for i in idx]
    table = c["table"].to(DEV).requires_grad_(True)
    if stacked:
        x = _place(c["images"][idx], offset).requires_grad_(True)
        out = apply_appearance(x, table, rows, c["center"])
        assert tuple(out.shape) == tuple(x.shape) and out.dtype == F32
        gx, gt = torch.autograd.grad(out, [x, table], _place(c["cot"][idx] * scale, offset))
        res = (out.detach(), gx, gt)
    else:
        xs = [_place(c["images"][i], offset).requires_grad_(True) for i in idx]
        outs = apply_appearance(xs, table, rows, c["center"])
        assert isinstance(outs, tuple) and len(outs) == len(idx)
        *gxs, gt = torch.autograd.grad(outs, xs + [table], [_place(c["cot"][i] * scale, offset) for i in idx])
        res = (torch.stack([o.detach() for o in outs]), torch.stack(gxs), gt)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in res)


def _c_backward(c, offset, want_images, want_table, views=None):
    """bags_appearance_backward itself, with real NULLs for what is not wanted, into buffers pre-filled with NaN."""
    idx = list(range(c["V"])) if views is None else list(views)
    assert len(idx) <= L.MAX_POSE_ROWS
    xs = [_place(c["images"][i], offset) for i in idx]
    gs = [_place(c["cot"][i], offset) for i in idx]
    table = c["table"].to(DEV)
    H, W = c["H"], c["W"]
    args = L.BagsAppearance(A.N, table.data_ptr(), len(idx), _row_table([c["rows"][i] for i in idx]), 3, H, W, c["center"][0], c["center"][1],
                            _ptr_field(xs))
    g_imgs = [_place(torch.full((3, H, W), float("nan")), offset) for _ in idx] if want_images else None
    g_table = torch.full((A.N, 16), float("nan"), device=DEV) if want_table else None
    ws = L.workspace(L.load().bags_appearance_workspace_size(len(idx), H, W), DEV) if want_table else None
    L.call("bags_appearance_backward", DEV, C.byref(args), L.ptr_table(gs), L.ptr(ws), ws.numel() if want_table else 0,
           L.ptr_table(g_imgs) if want_images else None, L.ptr(g_table))
    torch.cuda.synchronize()
    return (torch.stack(g_imgs).cpu() if want_images else None, g_table.cpu() if want_table else None)


def _check_table(c, g_table):
    """Listed rows in list order; every other row and column 15 are exact zeros."""
    rows = c["rows"]
    other = [r for r in range(A.N) if r not in rows]
    assert tuple(g_table.shape) == (A.N, 16) and torch.isfinite(g_table).all()
    assert g_table[other].abs().max().item() == 0.0 if other else True
    assert g_table[:, 15].abs().max().item() == 0.0
    return g_table[rows]


# ---------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("V", A.VIEWS)
@pytest.mark.parametrize("H,W", A.SHAPES, ids=["%dx%d" % s for s in A.SHAPES])
def test_values_against_float64(H, W, V, offset):
    """Output and dL/dimage per element, the 15 sums of every listed row per sum, within the bars of appearance_cases.bars; the
    test prints the margins (largest error over bar; table in profiles/appearance/NOTES.md: none above 0.16).  17 views are two
    launches each way; the aligned run of a shape with W % 4 == 0 is the vector path, every other run the scalar path."""
    c = A.make_case(H, W, V)
    out, g_images, g_table = _run(c, offset)
    g_rows = _check_table(c, g_table)
    assert torch.isfinite(out).all() and torch.isfinite(g_images).all()
    m = A.margins(H, W, V, out, g_images, g_rows)
    print("\n%dx%d V=%d %s: margins out %.3f  dL/dimage %.3f  dL/dtable %.3f" % (H, W, V, "offset" if offset else "aligned", *m))
    assert all(x <= 1.0 for x in m), m                        # (a NaN fails)


def test_bank_on_the_gpu_matches_the_host_copy():
    H, W, V = 37, 259, 2
    c = A.make_case(H, W, V)
    host, dev = AppearanceBank(A.N), AppearanceBank(A.N, DEV)
    with torch.no_grad():
        host.table.copy_(c["table"])
        dev.table.copy_(c["table"])
    assert dev.table.is_cuda and len(dev) == A.N
    xs_h = [c["images"][i].clone().requires_grad_(True) for i in range(V)]
    xs_d = [c["images"][i].to(DEV).requires_grad_(True) for i in range(V)]
    out_h = host.apply(xs_h, c["rows"], c["center"])
    out_d = dev.apply(xs_d, c["rows"], c["center"])
    sum((o * c["cot"][i]).sum() for i, o in enumerate(out_h)).backward()
    sum((o * c["cot"][i].to(DEV)).sum() for i, o in enumerate(out_d)).backward()
    bar = A.bars(H, W, V)
    assert all(o.grad_fn is not None and type(o.grad_fn).__name__.startswith("_Appearance") for o in out_d)
    for i in range(V):
        assert ((out_d[i].detach().cpu() - out_h[i].detach()).abs().double() <= bar[0][i]).all()
        assert ((xs_d[i].grad.cpu() - xs_h[i].grad).abs().double() <= bar[1][i]).all()
    d = (dev.table.grad.cpu() - host.table.grad).abs().double()
    assert (d[c["rows"]][:, A.USED] <= bar[2][:, A.USED]).all() and _check_table(c, dev.table.grad.cpu()) is not None
    # a single image and a single row
    one = dev.apply(xs_d[0].detach(), c["rows"][0], c["center"])
    assert tuple(one.shape) == (3, H, W) and torch.equal(one, out_d[0].detach())
    with pytest.raises(RuntimeError, match="AMD GPU"):
        dev.apply(xs_h[0].detach(), c["rows"][0])             # a host image into the GPU bank: refused, not copied


# ---------------------------------------------------------------------------------------------------------------- bitwise
@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("H,W", ((16, 64), (17, 67)))
def test_neutral_row_returns_its_input(H, W, offset):
    c = A.make_case(H, W, 2)
    bank = AppearanceBank(A.N, DEV)
    xs = [_place(c["images"][i], offset) for i in range(2)]
    with torch.no_grad():
        outs = bank.apply(xs, c["rows"], c["center"])
    assert all(torch.equal(o, x) and o.data_ptr() != x.data_ptr() for o, x in zip(outs, xs))


@pytest.mark.parametrize("V", (2, 17))
@pytest.mark.parametrize("H,W", VECTOR_SHAPES, ids=["%dx%d" % s for s in VECTOR_SHAPES])
def test_vector_path_equals_scalar_path(H, W, V):
    c = A.make_case(H, W, V)
    vec, sca = _run(c, offset=False), _run(c, offset=True)
    for a, b, what in zip(vec, sca, ("out", "dL/dimage", "dL/dtable")):
        assert torch.equal(a, b), what


def test_sequence_and_stack_give_the_same_bits():
    for offset in (False, True):
        c = A.make_case(*A.STRIDED, 17)
        seq, stk = _run(c, offset), _run(c, offset, stacked=True)
        for a, b, what in zip(seq, stk, ("out", "dL/dimage", "dL/dtable")):
            assert torch.equal(a, b), (what, offset)


def test_backward_repeats_bit_for_bit_also_on_a_side_stream():
    c = A.make_case(*A.STRIDED, 16)
    first, again = _run(c), _run(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _run(c)
    torch.cuda.current_stream().wait_stream(side)
    for a, b, d in zip(first, again, third):
        assert torch.equal(a, b) and torch.equal(a, d)


@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("H,W", ((17, 67), A.STRIDED), ids=("17x67", "strided"))
def test_each_output_alone_equals_the_full_call(H, W, offset):
    """Through the C entry with real NULLs; the buffers are pre-filled with NaN, so every element that must be written was, and
    the rows that are not listed and column 15 are exact zeros."""
    c = A.make_case(H, W, 16)
    gi_full, gt_full = _c_backward(c, offset, True, True)
    gi_only, none_t = _c_backward(c, offset, True, False)
    none_i, gt_only = _c_backward(c, offset, False, True)
    assert none_t is None and none_i is None
    assert torch.isfinite(gi_full).all() and torch.equal(gi_only, gi_full)
    _check_table(c, gt_full)
    assert torch.equal(gt_only, gt_full)
    _, g_images, g_table = _run(c, offset)                    # and autograd is that call
    assert torch.equal(g_images, gi_full) and torch.equal(g_table, gt_full)


@pytest.mark.parametrize("H,W", ((17, 67), A.STRIDED), ids=("17x67", "strided"))
def test_a_row_of_a_16_view_call_equals_its_own_call(H, W):
    c = A.make_case(H, W, 16)
    out, g_images, g_table = _run(c)
    for v in (0, 6, 15):
        o1, gi1, gt1 = _run(c, views=[v])
        r = c["rows"][v]
        assert torch.equal(o1[0], out[v]) and torch.equal(gi1[0], g_images[v]) and torch.equal(gt1[r], g_table[r])
        assert gt1[[i for i in range(A.N) if i != r]].abs().max().item() == 0.0


def test_a_scaled_cotangent_scales_the_gradients_exactly():
    c = A.make_case(*A.STRIDED, 2)
    _, g_images, g_table = _run(c)
    _, s_images, s_table = _run(c, scale=0.125)
    assert torch.equal(s_images, g_images * 0.125) and torch.equal(s_table, g_table * 0.125)


# ---------------------------------------------------------------------------------------------------------------- autograd
def test_table_step_between_forward_and_backward_raises_and_no_grad_keeps_nothing():
    bank = AppearanceBank(5, DEV)
    img = torch.rand(3, 64, 128, device=DEV)
    out = bank.apply(img, [3])
    with torch.no_grad():
        bank.table.add_(0.01)                                 # an optimizer step: the adjoint would re-read a table the forward did not see
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()
    del out
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    with torch.no_grad():
        out = bank.apply(img, [3])
    assert out.grad_fn is None and not out.requires_grad
    del img                                                   # nothing else holds the image: its bytes make up for the output's
    assert torch.cuda.memory_allocated() == held
    const = apply_appearance(torch.rand(3, 8, 8, device=DEV), bank.table.detach(), [0])
    assert const.grad_fn is None
    only_image = torch.rand(3, 8, 8, device=DEV, requires_grad=True)
    apply_appearance(only_image, bank.table.detach(), [0]).sum().backward()
    assert only_image.grad is not None and bank.table.grad is None


# ---------------------------------------------------------------------------------------------------------------- chain
def test_chain_resample_appearance_loss():
    """resample_image -> bank.apply -> fused_photometric_loss -> backward reaches image, ctrl_flow and bank.table.  Held to the same
    chain with appearance_torch in the middle: in float64 for the reference, in float32 on the GPU for the float32 PyTorch path's
    own error, by the rule of appearance_cases.bars (for the table the scale is sum |terms| of the 15 sums, from the reference's
    own cotangent).  Then one torch.optim.Adam([bank.table]) step moves the listed row's used columns and nothing else."""
    H, W, N, row = 40, 72, 6, 4
    g = torch.Generator().manual_seed(21)
    image0 = torch.rand(3, H, W, generator=g)
    gt = torch.rand(3, H, W, generator=g).to(DEV)
    gy, gx = torch.meshgrid(torch.linspace(-0.95, 0.95, 5), torch.linspace(-0.95, 0.95, 6), indexing="ij")
    ctrl0 = torch.stack((gx, gy), -1) + 0.02 * torch.randn(5, 6, 2, generator=g)
    table0 = torch.tensor(NEUTRAL).repeat(N, 1)
    table0[:, :15] += 0.2 * (torch.rand(N, 15, generator=g) * 2 - 1)
    center = (0.5 * W - 1.3, 0.5 * H + 0.8)

    def chain(middle):
        image, ctrl = image0.to(DEV).requires_grad_(True), ctrl0.to(DEV).requires_grad_(True)
        bank = AppearanceBank(N, DEV)
        with torch.no_grad():
            bank.table.copy_(table0)
        warped, _mask = resample_image(image, ctrl, (H, W), (H, W))
        shaded = middle(bank, warped)
        shaded.retain_grad()
        loss = fused_photometric_loss(shaded, gt)
        loss.backward()
        torch.cuda.synchronize()
        return bank, dict(loss=loss.detach().cpu(), image=image.grad.cpu(), ctrl=ctrl.grad.cpu(), table=bank.table.grad.cpu(),
                          warped=warped.detach().cpu(), cot=shaded.grad.cpu())

    bank, hip = chain(lambda b, x: b.apply(x, [row], center))
    _, t32 = chain(lambda b, x: appearance_torch(x, b.table[row], center))
    _, t64 = chain(lambda b, x: appearance_torch(x.double(), b.table[row].double(), center).float())
    assert torch.equal(hip["warped"], t64["warped"])
    eps = A.EPS32
    _, absum = A.sums_of_terms(t64["warped"][None], t64["cot"][None], table0[row][None], center)
    worst = {}
    for name in ("loss", "image", "ctrl", "table"):
        got, r32, r64 = hip[name].double(), t32[name].double(), t64[name].double()
        assert torch.isfinite(got).all() and got.abs().max().item() > 0, name
        assert (r64.abs() > 0).any() and torch.isfinite(r64).all(), name
        if name == "table":                                   # the listed row's 15 sums; everything else is checked to be zero below
            got, r32, r64, scale = got[row, A.USED], r32[row, A.USED], r64[row, A.USED], absum[0, A.USED]
        else:
            scale = 1 + r64.abs()
        bar = A.FACTOR * (r32 - r64).abs() + A.FLOOR_EPS * eps * scale
        worst[name] = float(((got - r64).abs() / bar).max())
    print("\nchain margins:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst       # (a NaN fails)
    others = [i for i in range(N) if i != row]
    assert hip["table"][others].abs().max().item() == 0.0 and hip["table"][row, 15].item() == 0.0 and (hip["table"][row, :15] != 0).all()
    before = bank.table.detach().clone()
    torch.optim.Adam([bank.table], lr=0.01).step()
    moved = (bank.table.detach() != before).cpu()
    assert moved[row, :15].all() and not moved[row, 15] and not moved[others].any()
