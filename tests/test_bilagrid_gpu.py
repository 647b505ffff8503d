"""GPU checks of the bilateral-grid step: bags_raster.apply_bilagrid / bilagrid_tv_loss / BilateralGridBank (csrc/bilagrid.hip)
against bilagrid_torch in float64 on the cases of tests/bilagrid_cases.py, held to that module's bars; the bitwise properties of its
two tile paths, its optional outputs and its sums; and the chain resample_image -> AppearanceBank.apply -> BilateralGridBank.apply
-> fused_photometric_loss + 10 * tv_loss.  (A thread is a pixel and every access a dword: there is no vector path to misalign.)"""
import ctypes as C

import pytest
import torch

import bilagrid_cases as B
from bags_raster import AppearanceBank, BilateralGridBank, _lib as L, appearance_torch, apply_bilagrid, bilagrid_torch, bilagrid_tv_loss, \
    bilagrid_tv_loss_torch
from bags_raster.appearance import _ptr_field
from bags_raster.distortion import resample_image
from bags_raster.loss import fused_photometric_loss
from bags_raster.pose_bank import _row_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
IDS = dict(ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
AUTO, DIRECT = L.BILAGRID_PATH_AUTO, L.BILAGRID_PATH_DIRECT
BIG = (16, 16, 8)


def _run(c, stacked=False, views=None, scale=1.0, path=AUTO):
    """Forward and backward through autograd: (out (V,3,H,W), dL/dimages (V,3,H,W), dL/dgrids (N,12,L,Gy,Gx)) on the host."""
    idx = list(range(c["V"])) if views is None else list(views)
    rows = [c["rows"][i] for i in idx]
    grids = c["grids"].to(DEV).requires_grad_(True)
    if stacked:
        x = c["images"][idx].to(DEV).requires_grad_(True)
        out = apply_bilagrid(x, grids, rows, path)
        assert tuple(out.shape) == tuple(x.shape) and out.dtype == F32
        gx, gg = torch.autograd.grad(out, [x, grids], (c["cot"][idx] * scale).to(DEV))
        res = (out.detach(), gx, gg)
    else:
        xs = [c["images"][i].to(DEV).requires_grad_(True) for i in idx]
        outs = apply_bilagrid(xs, grids, rows, path)
        assert isinstance(outs, tuple) and len(outs) == len(idx)
        *gxs, gg = torch.autograd.grad(outs, xs + [grids], [(c["cot"][i] * scale).to(DEV) for i in idx])
        res = (torch.stack([o.detach() for o in outs]), torch.stack(gxs), gg)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in res)


def _c_backward(c, want_images, want_grids, path=AUTO):
    """bags_bilagrid_backward itself, with real NULLs for what is not wanted, into buffers pre-filled with NaN."""
    V = c["V"]
    assert V <= L.MAX_POSE_ROWS
    xs = [c["images"][i].to(DEV) for i in range(V)]
    gs = [c["cot"][i].to(DEV) for i in range(V)]
    grids = c["grids"].to(DEV)
    (Gx, Gy, Lz), H, W = c["grid"], c["H"], c["W"]
    args = L.BagsBilagrid(B.N, grids.data_ptr(), V, _row_table(c["rows"]), 3, H, W, Gx, Gy, Lz, path, _ptr_field(xs))
    g_imgs = [torch.full((3, H, W), float("nan"), device=DEV) for _ in range(V)] if want_images else None
    g_grids = torch.full_like(grids, float("nan")) if want_grids else None
    L.call("bags_bilagrid_backward", DEV, C.byref(args), L.ptr_table(gs), None, 0, L.ptr_table(g_imgs) if want_images else None, L.ptr(g_grids))
    torch.cuda.synchronize()
    return (torch.stack(g_imgs).cpu() if want_images else None, g_grids.cpu() if want_grids else None)


def _check_grids(c, g_grids):
    """Finite everywhere; rows that are not listed are exact zeros.  Returns the listed rows in list order."""
    rows = c["rows"]
    other = [r for r in range(B.N) if r not in rows]
    assert tuple(g_grids.shape) == tuple(c["grids"].shape) and torch.isfinite(g_grids).all()
    assert g_grids[other].abs().max().item() == 0.0 if other else True
    return g_grids[rows]


# ---------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("V", B.VIEWS)
@pytest.mark.parametrize("H,W", B.SHAPES, **IDS)
@pytest.mark.parametrize("grid", B.GRIDS, **IDS)
def test_values_against_float64(grid, H, W, V):
    """Output and dL/dimage per element, dL/dgrid per element of every listed row, within the bars of bilagrid_cases.bars; the test
    prints the margins (largest error over bar; table in profiles/bilagrid/NOTES.md).  17 views are two launches each way.  A vertex
    no pixel reaches has a zero bar: it must be an exact zero."""
    c = B.make_case(grid, H, W, V)
    out, g_images, g_grids = _run(c)
    g_rows = _check_grids(c, g_grids)
    assert torch.isfinite(out).all() and torch.isfinite(g_images).all()
    unreached = B.term_sums(grid, H, W, V)[1] == 0
    assert (g_rows[unreached] == 0).all()
    m = B.margins(grid, H, W, V, out, g_images, g_rows)
    print("\n%s %dx%d V=%d: margins out %.3f  dL/dimage %.3f  dL/dgrid %.3f" % ("x".join(map(str, grid)), H, W, V, *m))
    assert all(x <= 1.0 for x in m), m                        # (a NaN fails)


@pytest.mark.parametrize("n", (1, B.N))
@pytest.mark.parametrize("grid", B.GRIDS, **IDS)
def test_tv_value_and_gradient_against_float64(grid, n):
    grids, cot = B.tv_case(grid, n)
    x = grids.to(DEV).requires_grad_(True)
    loss = bilagrid_tv_loss(x)
    assert loss.dtype == F32 and loss.dim() == 0
    (gx,) = torch.autograd.grad(loss, x, torch.tensor(cot, device=DEV))
    (l64, g64), (lbar, gbar) = B.tv_reference(grid, n), B.tv_bars(grid, n)
    el, eg = abs(loss.item() - l64.item()), (gx.cpu().double() - g64).abs()
    print("\n%s N=%d: tv %.6g err %.3g bar %.3g; gradient worst err/bar %.3f" % (
        "x".join(map(str, grid)), n, l64.item(), el, lbar.item(), float((eg / gbar.clamp(min=1e-300)).max())))
    assert el <= lbar.item() and (eg <= gbar).all()
    # repeats bit for bit; a neutral bank has zero TV and an exactly zero gradient
    loss2 = bilagrid_tv_loss(x)
    (gx2,) = torch.autograd.grad(loss2, x, torch.tensor(cot, device=DEV))
    assert torch.equal(loss2, loss.detach()) and torch.equal(gx2, gx)
    bank = BilateralGridBank(n, grid, DEV)
    tv = bank.tv_loss()
    tv.backward()
    assert tv.item() == 0.0 and bank.grids.grad.abs().max().item() == 0.0
    assert bilagrid_tv_loss(grids.to(DEV)).grad_fn is None


def test_bank_on_the_gpu_matches_the_host_copy():
    grid, H, W, V = (5, 4, 3), 37, 259, 2
    c = B.make_case(grid, H, W, V)
    host, dev = BilateralGridBank(B.N, grid), BilateralGridBank(B.N, grid, DEV)
    with torch.no_grad():
        host.grids.copy_(c["grids"])
        dev.grids.copy_(c["grids"])
    assert dev.grids.is_cuda and len(dev) == B.N
    xs_h = [c["images"][i].clone().requires_grad_(True) for i in range(V)]
    xs_d = [c["images"][i].to(DEV).requires_grad_(True) for i in range(V)]
    out_h, out_d = host.apply(xs_h, c["rows"]), dev.apply(xs_d, c["rows"])
    sum((o * c["cot"][i]).sum() for i, o in enumerate(out_h)).backward()
    sum((o * c["cot"][i].to(DEV)).sum() for i, o in enumerate(out_d)).backward()
    bar = B.bars(grid, H, W, V)
    assert all(o.grad_fn is not None and type(o.grad_fn).__name__.startswith("_Bilagrid") for o in out_d)
    for i in range(V):                                        # both are within a bar of float64: within two of each other
        assert ((out_d[i].detach().cpu() - out_h[i].detach()).abs().double() <= 2 * bar[0][i]).all()
        assert ((xs_d[i].grad.cpu() - xs_h[i].grad).abs().double() <= 2 * bar[1][i]).all()
    d = (dev.grids.grad.cpu() - host.grids.grad).abs().double()
    assert (d[c["rows"]] <= 2 * bar[2]).all() and _check_grids(c, dev.grids.grad.cpu()) is not None
    one = dev.apply(xs_d[0].detach(), c["rows"][0])
    assert tuple(one.shape) == (3, H, W) and torch.equal(one, out_d[0].detach())
    A = dev.affine(xs_d[0].detach(), c["rows"][0])
    assert A.is_cuda and tuple(A.shape) == (3, 4, H, W)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        dev.apply(xs_h[0].detach(), c["rows"][0])             # a host image into the GPU bank: refused, not copied
    with pytest.raises(ValueError, match="bilagrid_torch"):
        apply_bilagrid(xs_d[0].detach(), torch.zeros(1, 12, 17, 4, 4, device=DEV), [0])


# ---------------------------------------------------------------------------------------------------------------- bitwise
@pytest.mark.parametrize("H,W", ((16, 64), (17, 67), (3, 5)), **IDS)
@pytest.mark.parametrize("grid", (BIG, (2, 3, 2)), **IDS)
def test_neutral_bank_returns_its_input(grid, H, W):
    c = B.make_case(grid, H, W, 2)
    bank = BilateralGridBank(B.N, grid, DEV)
    xs = [c["images"][i].to(DEV) for i in range(2)]
    with torch.no_grad():
        outs = bank.apply(xs, c["rows"])
    assert all(torch.equal(o, x) and o.data_ptr() != x.data_ptr() for o, x in zip(outs, xs))


@pytest.mark.parametrize("V", (2, 17))
@pytest.mark.parametrize("grid,H,W", ((BIG, *B.DERIVED), ((5, 4, 3), *B.DERIVED), ((2, 3, 2), 37, 259), ((5, 4, 3), 17, 67)), **IDS)
def test_staged_tiles_equal_direct_tiles(grid, H, W, V):
    """Where tiles stage their vertices in LDS, the same call with every tile reading the grid directly gives the same bits."""
    assert B.tile_paths(grid, H, W)[0] > 0
    c = B.make_case(grid, H, W, V)
    auto, direct = _run(c, path=AUTO), _run(c, path=DIRECT)
    for a, b, what in zip(auto, direct, ("out", "dL/dimage", "dL/dgrid")):
        assert torch.equal(a, b), what


def test_sequence_and_stack_give_the_same_bits():
    c = B.make_case(BIG, *B.DERIVED, 17)
    seq, stk = _run(c), _run(c, stacked=True)
    for a, b, what in zip(seq, stk, ("out", "dL/dimage", "dL/dgrid")):
        assert torch.equal(a, b), what


def test_backward_repeats_bit_for_bit_also_on_a_side_stream():
    c = B.make_case((5, 4, 3), *B.DERIVED, 16)
    first, again = _run(c), _run(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _run(c)
    torch.cuda.current_stream().wait_stream(side)
    for a, b, d in zip(first, again, third):
        assert torch.equal(a, b) and torch.equal(a, d)


@pytest.mark.parametrize("grid,H,W", ((BIG, 3, 5), ((5, 4, 3), *B.DERIVED), (BIG, 17, 67)), **IDS)
def test_each_output_alone_equals_the_full_call(grid, H, W):
    """Through the C entry with real NULLs; the buffers are pre-filled with NaN, so every element that must be written was: rows
    that are not listed and vertices no pixel reaches are exact zeros."""
    c = B.make_case(grid, H, W, 16)
    gi_full, gg_full = _c_backward(c, True, True)
    gi_only, none_g = _c_backward(c, True, False)
    none_i, gg_only = _c_backward(c, False, True)
    assert none_g is None and none_i is None
    assert torch.isfinite(gi_full).all() and torch.equal(gi_only, gi_full)
    g_rows = _check_grids(c, gg_full)
    unreached = B.term_sums(grid, H, W, 16)[1] == 0
    assert (g_rows[unreached] == 0).all() and ((H, W) != (3, 5) or unreached.float().mean() > 0.5)
    assert torch.equal(gg_only, gg_full)
    _, g_images, g_grids = _run(c)                            # and autograd is that call
    assert torch.equal(g_images, gi_full) and torch.equal(g_grids, gg_full)


@pytest.mark.parametrize("grid,H,W", ((BIG, 17, 67), ((5, 4, 3), *B.DERIVED)), **IDS)
def test_a_row_of_a_16_view_call_equals_its_own_call(grid, H, W):
    c = B.make_case(grid, H, W, 16)
    out, g_images, g_grids = _run(c)
    for v in (0, 6, 15):
        o1, gi1, gg1 = _run(c, views=[v])
        r = c["rows"][v]
        assert torch.equal(o1[0], out[v]) and torch.equal(gi1[0], g_images[v]) and torch.equal(gg1[r], g_grids[r])
        assert gg1[[i for i in range(B.N) if i != r]].abs().max().item() == 0.0


def test_a_scaled_cotangent_scales_the_gradients_exactly():
    c = B.make_case(BIG, *B.DERIVED, 2)
    _, g_images, g_grids = _run(c)
    _, s_images, s_grids = _run(c, scale=0.125)
    assert torch.equal(s_images, g_images * 0.125) and torch.equal(s_grids, g_grids * 0.125)


# ---------------------------------------------------------------------------------------------------------------- autograd
def test_grid_step_between_forward_and_backward_raises_and_no_grad_keeps_nothing():
    bank = BilateralGridBank(5, (5, 4, 3), DEV)
    img = torch.rand(3, 64, 128, device=DEV)
    out = bank.apply(img, [3])
    with torch.no_grad():
        bank.grids.add_(0.01)                                 # an optimizer step: the adjoint would re-read grids the forward did not see
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
    const = apply_bilagrid(torch.rand(3, 8, 8, device=DEV), bank.grids.detach(), [0])
    assert const.grad_fn is None
    only_image = torch.rand(3, 8, 8, device=DEV, requires_grad=True)
    apply_bilagrid(only_image, bank.grids.detach(), [0]).sum().backward()
    assert only_image.grad is not None and bank.grids.grad is None


# ---------------------------------------------------------------------------------------------------------------- chain
def test_chain_resample_appearance_bilagrid_loss_and_tv():
    """resample_image -> AppearanceBank.apply -> BilateralGridBank.apply -> fused_photometric_loss + 10 * tv_loss -> backward reaches
    image, ctrl_flow, the appearance table and the grids.  Held to the same chain with the PyTorch statements in the middle: in
    float64 for the reference, in float32 on the GPU for the float32 PyTorch path's own error, by the rule of bilagrid_cases.bars
    (for the grids the scale is sum |terms| from the reference's own cotangent, plus the TV gradient's).  Then one
    torch.optim.Adam([bank.grids]) step moves the listed row and leaves every other row neutral bit for bit."""
    H, W, N, row, grid = 40, 72, 6, 4, (5, 4, 3)
    g = torch.Generator().manual_seed(23)
    image0 = torch.rand(3, H, W, generator=g)
    gt = torch.rand(3, H, W, generator=g).to(DEV)
    gy, gx = torch.meshgrid(torch.linspace(-0.95, 0.95, 5), torch.linspace(-0.95, 0.95, 6), indexing="ij")
    ctrl0 = torch.stack((gx, gy), -1) + 0.02 * torch.randn(5, 6, 2, generator=g)
    table0 = AppearanceBank(N).table.detach().clone()
    table0[:, :15] += 0.1 * (torch.rand(N, 15, generator=g) * 2 - 1)
    neutral = BilateralGridBank(N, grid).grids.detach().clone()
    grids0 = neutral.clone()
    grids0[row] += 0.2 * (torch.rand(12, grid[2], grid[1], grid[0], generator=g) * 2 - 1)        # the other rows stay neutral

    def chain(appearance, slice_, tv):
        image, ctrl = image0.to(DEV).requires_grad_(True), ctrl0.to(DEV).requires_grad_(True)
        app, bank = AppearanceBank(N, DEV), BilateralGridBank(N, grid, DEV)
        with torch.no_grad():
            app.table.copy_(table0)
            bank.grids.copy_(grids0)
        warped, _mask = resample_image(image, ctrl, (H, W), (H, W))
        exposed = appearance(app, warped)
        exposed.retain_grad()
        shaded = slice_(bank, exposed)
        shaded.retain_grad()
        loss = fused_photometric_loss(shaded, gt) + 10 * tv(bank)
        loss.backward()
        torch.cuda.synchronize()
        return bank, dict(loss=loss.detach().cpu(), image=image.grad.cpu(), ctrl=ctrl.grad.cpu(), table=app.table.grad.cpu(),
                          grids=bank.grids.grad.cpu(), exposed=exposed.detach().cpu(), cot=shaded.grad.cpu())

    bank, hip = chain(lambda a, x: a.apply(x, [row]), lambda b, x: b.apply(x, [row]), lambda b: b.tv_loss())
    _, t32 = chain(lambda a, x: appearance_torch(x, a.table[row]), lambda b, x: bilagrid_torch(x, b.grids[row]), lambda b: bilagrid_tv_loss_torch(b.grids))
    _, t64 = chain(lambda a, x: appearance_torch(x.double(), a.table[row].double()).float(),
                   lambda b, x: bilagrid_torch(x.double(), b.grids[row].double()).float(), lambda b: bilagrid_tv_loss_torch(b.grids.double()).float())
    eps = B.EPS32
    _, grid_abs = B.sums_of_terms(t64["exposed"][None], t64["cot"][None], grids0[row][None])
    x = grids0.double()
    tv_abs = torch.zeros_like(x)                              # sum |terms| of 10 * the TV gradient (bilagrid_cases.tv_bars)
    for dim, size, others in ((4, grid[0], grid[1] * grid[2]), (3, grid[1], grid[0] * grid[2]), (2, grid[2], grid[0] * grid[1])):
        d = (x.narrow(dim, 1, size - 1) - x.narrow(dim, 0, size - 1)).abs() * (10 * 2 / (N * 12 * (size - 1) * others))
        tv_abs.narrow(dim, 0, size - 1).add_(d)
        tv_abs.narrow(dim, 1, size - 1).add_(d)
    worst = {}
    for name in ("loss", "image", "ctrl", "table", "grids"):
        got, r32, r64 = hip[name].double(), t32[name].double(), t64[name].double()
        assert torch.isfinite(got).all() and got.abs().max().item() > 0, name
        assert (r64.abs() > 0).any() and torch.isfinite(r64).all(), name
        if name == "grids":                                   # the listed row; everything else is checked to be zero below
            got, r32, r64, scale = got[row], r32[row], r64[row], grid_abs[0] + tv_abs[row]
        elif name == "table":
            got, r32, r64 = got[row, :15], r32[row, :15], r64[row, :15]
            scale = 1 + r64.abs()
        else:
            scale = 1 + r64.abs()
        bar = B.FACTOR * (r32 - r64).abs() + B.FLOOR_EPS * eps * scale
        worst[name] = float(((got - r64).abs() / bar).max())
    print("\nchain margins:", {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst       # (a NaN fails)
    others = [i for i in range(N) if i != row]
    assert hip["grids"][others].abs().max().item() == 0.0     # the slice lists one row, and the TV of a neutral row has zero gradient
    torch.optim.Adam([bank.grids], lr=0.01).step()
    after = bank.grids.detach().cpu()
    assert torch.equal(after[others], neutral[others]) and (after[row] != grids0[row]).float().mean().item() > 0.9
