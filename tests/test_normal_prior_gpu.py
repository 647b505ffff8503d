"""GPU checks of the normal prior: bags_raster.normal_prior_loss / depth_to_normal (csrc/normal_prior.hip) against
normal_prior_loss_torch in float64 on the cases of tests/normal_prior_cases.py, held to that module's bars; the bitwise properties
of its sums and its optional outputs; the degenerate views; depth_to_normal; and the chain rasterizer -> normal_prior_loss ->
backward."""
import ctypes as C
import math

import pytest
import torch

import normal_prior_cases as P
from bags_raster import _lib as L, depth_to_normal, depth_to_normal_torch, normal_prior_loss, normal_prior_loss_torch, pinhole_of
from bags_raster.normal_prior import MODES, _pinhole_field, _ptr_field

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
NAMES = ("loss", "dL/dD", "dL/dA")
CHAIN_MIN_WEIGHT = 0.87                                      # of the chain through the real operator: the scene's weights lie in
                                                             # [0.861, 0.955], three pixels below 0.87 (depth_prior_cases)


def _place(t, offset):
    """``t`` as a float32 GPU tensor: at the start of an allocation, or -- ``offset`` -- as a view 4 bytes into a larger one."""
    n = t.numel()
    buf = torch.empty(n + 4, dtype=F32, device=DEV)
    v = (buf[1:1 + n] if offset else buf[:n]).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 if offset else 0) and v.is_contiguous()
    return v


def _maps(c, idx, offset):
    return ([_place(c["D"][i], offset) for i in idx], [_place(c["A"][i], offset) for i in idx],
            [_place(c["prior"][i], offset) for i in idx], [_place(c["mask"][i], offset) for i in idx])


def _run(c, offset=False, views=None, scale=1.0, max_jump=P.MAX_JUMP):
    """Forward and backward through autograd for L = sum cot_v loss_v: (loss (V,), dL/dD (V,1,H,W), dL/dA (V,1,H,W), count (V,)) on
    the host."""
    idx = list(range(c["V"])) if views is None else list(views)
    Ds, As, ps, ms = _maps(c, idx, offset)
    for t in Ds + As:
        t.requires_grad_(True)
    loss, count = normal_prior_loss(Ds, As, ps, c["pinhole"][idx], ms, mode=c["mode"], min_weight=P.MIN_WEIGHT, max_jump=max_jump)
    assert tuple(loss.shape) == (len(idx),) == tuple(count.shape) and loss.dtype == F32 and not count.requires_grad
    grads = torch.autograd.grad(loss, Ds + As, (c["cot"][idx] * scale).to(DEV))
    torch.cuda.synchronize()
    n = len(idx)
    return loss.detach().cpu(), torch.stack(grads[:n]).cpu(), torch.stack(grads[n:]).cpu(), count.cpu()


def _c_calls(c, offset, want_depth, want_weights):
    """bags_normal_prior_forward and _backward themselves, with real NULLs for what is not wanted, into buffers pre-filled with NaN."""
    idx = list(range(c["V"]))
    assert len(idx) <= L.MAX_POSE_ROWS
    Ds, As, ps, ms = _maps(c, idx, offset)
    H, W, n = c["H"], c["W"], len(idx)
    args = L.BagsNormalPrior(MODES[c["mode"]], H, W, P.MIN_WEIGHT, P.MAX_JUMP, n, _pinhole_field([tuple(r) for r in c["pinhole"].tolist()]),
                             _ptr_field(Ds), _ptr_field(As), _ptr_field(ps), _ptr_field(ms))
    loss, count = torch.full((n,), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)
    stats = torch.full((n, L.NORMAL_PRIOR_STATS), float("nan"), dtype=F64, device=DEV)
    ws = L.workspace(L.load().bags_normal_prior_workspace_size(n, H, W), DEV)
    ws.fill_(255)                                            # NaN bit patterns: every partial row that is read was written
    L.call("bags_normal_prior_forward", DEV, C.byref(args), L.ptr(ws), ws.numel(), L.ptr(loss), L.ptr(count), L.ptr(stats))
    g_d = [_place(torch.full((1, H, W), float("nan")), offset) for _ in idx] if want_depth else None
    g_a = [_place(torch.full((1, H, W), float("nan")), offset) for _ in idx] if want_weights else None
    g_loss = c["cot"].to(DEV)
    L.call("bags_normal_prior_backward", DEV, C.byref(args), L.ptr(stats), L.ptr(g_loss),
           L.ptr_table(g_d) if want_depth else None, L.ptr_table(g_a) if want_weights else None)
    torch.cuda.synchronize()
    return (loss.cpu(), torch.stack(g_d).cpu() if want_depth else None, torch.stack(g_a).cpu() if want_weights else None, count.cpu(),
            stats.cpu())


def _check_values(H, W, V, mode, offset, max_jump):
    c = P.make_case(H, W, V, mode)
    res = _run(c, offset, max_jump=max_jump)
    assert all(torch.isfinite(t).all() for t in res)
    ref = P.reference(H, W, V, mode, max_jump)
    assert ((res[3].double() - ref[3]).abs() <= P.EPS32 * ref[3]).all()                  # count = cnt, rounded once
    m = P.margins(H, W, V, mode, res[:3], max_jump)
    print("\n%dx%d V=%d %s max_jump=%s %s: margins %s" % (H, W, V, mode, max_jump, "offset" if offset else "aligned",
                                                          "  ".join("%s %.3f" % (n, x) for n, x in zip(NAMES, m))))
    assert all(x <= 1.0 for x in m), m                        # (a NaN fails; where a bar is 0 the value must be an exact zero)


# ---------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("V", P.VIEWS)
@pytest.mark.parametrize("H,W", P.SHAPES, ids=["%dx%d" % s for s in P.SHAPES])
def test_values_against_float64(H, W, V, mode, offset):
    """Loss per view, dL/dD and dL/dA per pixel within the bars of normal_prior_cases.bars with max_jump = 0.25; the test prints the
    margins (largest error over bar; profiles/normal_prior/NOTES.md has their maximum).  Pixels no valid centre reads are exact
    zeros (their bars are 0).  17 views are two launches of each kernel."""
    _check_values(H, W, V, mode, offset, P.MAX_JUMP)


@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("V", P.VIEWS)
@pytest.mark.parametrize("H,W", ((17, 67), P.SEAM), ids=("17x67", "seam"))
def test_values_with_the_guard_off(H, W, V, mode, offset):
    _check_values(H, W, V, mode, offset, math.inf)


# ---------------------------------------------------------------------------------------------------------------- bitwise
def _same(a, b, what=""):
    for x, y, name in zip(a, b, NAMES + ("count",)):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert torch.equal(x, y), (what, name)


@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("H,W", ((17, 67), P.SEAM), ids=("17x67", "seam"))
def test_a_view_of_a_16_view_call_equals_its_own_call(H, W, mode):
    c = P.make_case(H, W, 16, mode)
    loss, gD, gA, count = _run(c)
    for v in (0, 6, 15):
        l1, d1, a1, n1 = _run(c, views=[v])
        assert torch.equal(l1[0], loss[v]) and torch.equal(n1[0], count[v]) and torch.equal(d1[0], gD[v]) and torch.equal(a1[0], gA[v])


@pytest.mark.parametrize("mode", P.MODES)
def test_repeats_bit_for_bit_also_on_a_side_stream(mode):
    c = P.make_case(*P.SEAM, 16, mode)
    first, again = _run(c), _run(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _run(c)
    torch.cuda.current_stream().wait_stream(side)
    _same(first, again)
    _same(first, third)


@pytest.mark.parametrize("mode", P.MODES)
def test_a_scaled_cotangent_scales_the_gradients_exactly(mode):
    c = P.make_case(*P.SEAM, 2, mode)
    full, eighth = _run(c), _run(c, scale=0.125)
    assert torch.equal(eighth[0], full[0]) and torch.equal(eighth[1], full[1] * 0.125) and torch.equal(eighth[2], full[2] * 0.125)
    assert full[1].abs().max() > 0 and full[2].abs().max() > 0


@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("mode", P.MODES)
@pytest.mark.parametrize("H,W", ((17, 67), P.SEAM), ids=("17x67", "seam"))
def test_each_output_alone_equals_the_full_call(H, W, mode, offset):
    """Through the C entries with real NULLs; the buffers are pre-filled with NaN, so every element that must be written was."""
    c = P.make_case(H, W, 16, mode)
    full = _c_calls(c, offset, True, True)
    assert all(torch.isfinite(t).all() for t in full)
    only_d, only_a = _c_calls(c, offset, True, False), _c_calls(c, offset, False, True)
    assert only_d[2] is None and only_a[1] is None
    assert torch.equal(only_d[1], full[1]) and torch.equal(only_a[2], full[2])
    assert torch.equal(only_a[4], full[4]) and tuple(full[4].shape) == (16, 2) and torch.equal(full[4][:, 1].float(), full[3])
    assert torch.equal(full[4][:, 0], 1.0 / full[4][:, 1])
    _same(_run(c, offset), full[:4])                          # and autograd is those calls


# ---------------------------------------------------------------------------------------------------------------- degenerate views
@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("mode", P.MODES)
def test_degenerate_views(mode, offset):
    """Loss 0, count 0, zero gradients and finite values for the views normal_prior_cases.degenerate_case marks; every view within
    the bars of the rule; and the twelve ordinary views bit for bit what a call without the four gives."""
    c = P.degenerate_case(mode)
    res = _run(c, offset)
    assert all(torch.isfinite(t).all() for t in res)
    for v in c["degenerate"]:
        assert res[0][v] == 0 and res[3][v] == 0 and res[1][v].abs().max() == 0 and res[2][v].abs().max() == 0, v
    k = P.DEGENERATE_VIEWS
    v = k["one_centre"]
    assert res[3][v] == 0.625 and res[0][v] > 0 and int((res[1][v] != 0).sum()) == 4 == int((res[2][v] != 0).sum())
    r64, r32 = P.run_torch(c, F64), P.run_torch(c, F32)
    m = P.margins_of(P.bars_of(c, r64, r32), r64, res[:3])
    print("\ndegenerate %s: margins %s" % (mode, m))
    assert all(x <= 1.0 for x in m), m
    keep = [v for v in range(16) if v not in k.values()]
    without = _run(c, offset, views=keep)
    assert all(torch.equal(without[i], res[i][keep]) for i in range(4))


# ---------------------------------------------------------------------------------------------------------------- depth_to_normal
@pytest.mark.parametrize("max_jump", (P.MAX_JUMP, math.inf), ids=("guard", "no-guard"))
@pytest.mark.parametrize("H,W", P.SHAPES, ids=["%dx%d" % s for s in P.SHAPES])
def test_depth_to_normal(H, W, max_jump):
    """valid is the statement's; normal within 4 x what the float32 statement loses against the float64 statement plus 16 float32
    epsilons per component (a unit vector: scale 1); zeros where not valid."""
    c = P.make_case(H, W, 2, "cos")
    for v in range(2):
        pin = c["pinhole"][v]
        n64, ok64 = depth_to_normal_torch(c["D"][v].double(), c["A"][v].double(), pin, min_weight=P.MIN_WEIGHT, max_jump=max_jump)
        n32, ok32 = depth_to_normal_torch(c["D"][v], c["A"][v], pin, min_weight=P.MIN_WEIGHT, max_jump=max_jump)
        normal, valid = depth_to_normal(_place(c["D"][v], bool(v)), _place(c["A"][v], bool(v)), pin, min_weight=P.MIN_WEIGHT, max_jump=max_jump)
        torch.cuda.synchronize()
        assert normal.dtype == F32 and tuple(normal.shape) == (3, H, W) and valid.dtype == torch.bool and tuple(valid.shape) == (H, W)
        assert torch.equal(ok32, ok64) and torch.equal(valid.cpu(), ok64)
        assert torch.equal(ok64, P._pieces(c, max_jump)["geometric"][v])
        bar = P.FACTOR * (n32.double() - n64).abs() + P.FLOOR_EPS * P.EPS32
        err = (normal.cpu().double() - n64).abs()
        assert (err <= bar).all(), float((err / bar).max())
        assert normal.cpu()[:, ~ok64].abs().max().item() == 0.0 if (~ok64).any() else True
        if ok64.any():
            assert ((normal.cpu()[:, ok64].double().norm(dim=0) - 1).abs() <= 4 * P.EPS32).all()


# ---------------------------------------------------------------------------------------------------------------- autograd
def test_no_grad_keeps_nothing_and_constants_give_no_graph():
    c = P.make_case(37, 259, 2, "cos")
    Ds, As, ps, ms = _maps(c, [0, 1], False)
    pin = c["pinhole"]
    loss, count = normal_prior_loss(Ds, As, ps, pin, ms)
    assert loss.grad_fn is None and not loss.requires_grad and count.grad_fn is None             # constant inputs
    del loss, count
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    for t in Ds + As:
        t.requires_grad_(True)
    with torch.no_grad():
        loss, count = normal_prior_loss(Ds, As, ps, pin, ms)
    assert loss.grad_fn is None and not loss.requires_grad
    del loss, count
    assert torch.cuda.memory_allocated() == held              # nothing was saved
    loss, count = normal_prior_loss(Ds, As, ps, pin, ms)
    assert loss.grad_fn is not None and type(loss.grad_fn).__name__.startswith("_NormalPrior") and not count.requires_grad
    only_depth = normal_prior_loss(Ds[0], As[0].detach(), ps[0], pin[0])[0]
    only_depth.sum().backward()
    assert Ds[0].grad is not None and As[0].grad is None
    # the adjoint re-reads the maps: an in-place write between forward and backward raises
    D2 = Ds[1].detach().clone().requires_grad_(True)
    D2w = D2 * 1.0
    loss = normal_prior_loss(D2w, As[1].detach(), ps[1], pin[1])[0]
    D2w.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.sum().backward()
    with pytest.raises(RuntimeError, match="AMD GPU"):
        normal_prior_loss(c["D"][0], As[0], ps[0], pin[0])    # a host map into the HIP path: refused, not copied
    with pytest.raises(TypeError, match=r"\.float\(\)"):
        normal_prior_loss(Ds[0], As[0], ps[0], pin[0], ms[0] > 0)
    with pytest.raises(ValueError, match="GPU tensor"):
        normal_prior_loss(Ds[0], As[0], ps[0], pin[0].to(DEV))
    with pytest.raises(ValueError, match="GPU tensor"):
        normal_prior_loss(Ds, As, ps, [pin[0], pin[1].to(DEV)])
    with pytest.raises(ValueError, match="GPU tensor"):
        depth_to_normal(Ds[0].detach(), As[0].detach(), pin[0].to(DEV))


# ---------------------------------------------------------------------------------------------------------------- chain
@pytest.mark.parametrize("mode", P.MODES)
def test_chain_with_the_real_operator(mode):
    """rasterize(depth_weights_grad=True) -> normal_prior_loss with pinhole_of(intrinsic) -> backward reaches means3D, the opacities
    and the viewmatrix.  Held to the same chain with normal_prior_loss_torch in the middle -- in float64 for the reference, in float32
    on the GPU for the float32 path's own error -- by the rule: 4 x that error plus 16 float32 epsilons x (1 + |reference|) per
    element; the rasterizer is the same on all three sides.  The prior is the scene's own normals, perturbed."""
    from bags_raster import GaussianRasterizer
    from scenes import camera_tensors, hip_settings, make_case
    scene, cam = make_case(24, 32, 32, 3.0, 1, seed=5, dist=3.0)
    H, W = cam.image_height, cam.image_width
    pin = pinhole_of(camera_tensors(cam)["intrinsic"], H, W)

    def render():
        t = {k: v.to(DEV).clone().requires_grad_(True) for k, v in scene.items()}
        ct = {k: v.clone().requires_grad_(True) for k, v in camera_tensors(cam, DEV).items()}
        n = t["means3D"].shape[0]
        st = hip_settings(cam, 1, DEV, tensors=ct)._replace(depth_weights_grad=True)
        outs = GaussianRasterizer(st)(means3D=t["means3D"], means2D=torch.zeros(n, 3, device=DEV, requires_grad=True),
                                      means2D_densify=torch.zeros(n, 3, device=DEV, requires_grad=True),
                                      shift_factors=torch.zeros(3, device=DEV, requires_grad=True), shs=t["shs"], colors_precomp=None,
                                      opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"], cov3D_precomp=None)
        return t, ct, outs[2], outs[3]

    with torch.no_grad():
        _, _, depth0, weights0 = render()
    gap = (weights0 - CHAIN_MIN_WEIGHT).abs().min().item()
    n0, ok0 = depth_to_normal_torch(depth0.double().cpu(), weights0.double().cpu(), pin, min_weight=CHAIN_MIN_WEIGHT)
    g = torch.Generator().manual_seed(31)
    prior = n0 + 0.2 * torch.randn(3, H, W, generator=g, dtype=F64).clamp(-3, 3)
    prior = torch.where(ok0[None], prior, torch.tensor((0.0, 0.0, -1.0), dtype=F64).view(3, 1, 1))
    prior[:, torch.rand(H, W, generator=g) < 0.05] = 0.0
    mask = torch.where(torch.rand(H, W, generator=g) < 0.1, 0.0, 1.0) * (0.25 + 0.75 * torch.rand(H, W, generator=g))
    prior, mask = prior.float().to(DEV), mask.to(DEV)
    valid = ok0.to(DEV) & (mask > 0) & ((prior * prior).sum(0) > 0.25)
    print("\nchain %s: |weights - min_weight| >= %.3g, valid share %.3f" % (mode, gap, valid.float().mean().item()))
    assert gap >= 5e-4 and valid.float().mean().item() >= 0.25

    def chain(middle):
        t, ct, depth, weights = render()
        assert depth.requires_grad and weights.requires_grad
        loss, count = middle(depth, weights, dict(mode=mode, min_weight=CHAIN_MIN_WEIGHT))
        loss.sum().backward()
        torch.cuda.synchronize()
        return dict(loss=loss.detach().double().cpu(), count=count.double().cpu(), means3D=t["means3D"].grad.cpu(),
                    opacities=t["opacities"].grad.cpu(), viewmatrix=ct["viewmatrix"].grad.cpu())

    hip = chain(lambda d, a, kw: normal_prior_loss(d, a, prior, pin, mask, **kw))
    t32 = chain(lambda d, a, kw: normal_prior_loss_torch(d, a, prior, pin, mask, **kw))
    t64 = chain(lambda d, a, kw: normal_prior_loss_torch(d.double(), a.double(), prior.double(), pin, mask.double(), **kw))
    assert t64["count"].item() > 0 and all(abs(r["count"].item() - t64["count"].item()) <= P.EPS32 * t64["count"].item() for r in (hip, t32))
    worst = {}
    for name in ("loss", "means3D", "opacities", "viewmatrix"):
        got, r32, r64 = hip[name].double(), t32[name].double(), t64[name].double()
        assert torch.isfinite(got).all() and got.abs().max().item() > 0 and r64.abs().max().item() > 0, name
        bar = P.FACTOR * (r32 - r64).abs() + P.FLOOR_EPS * P.EPS32 * (1 + r64.abs())
        worst[name] = float(((got - r64).abs() / bar).max())
    print("chain %s margins:" % mode, {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst       # (a NaN fails)
