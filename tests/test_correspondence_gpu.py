"""GPU checks of the correspondence loss: bags_raster.correspondence_loss / reproject_pixels (csrc/correspondence.hip) against
correspondence_loss_torch in float64 on the cases of tests/correspondence_cases.py, held to that module's bars; the bitwise
properties of its sums and its optional outputs; the degenerate pairs; reproject_pixels; and the chain render_views ->
correspondence_loss -> backward."""
import ctypes as C

import pytest
import torch

import correspondence_cases as P
from bags_raster import _lib as L, correspondence_loss, pinhole_of, reproject_pixels, reproject_pixels_torch
from bags_raster.correspondence import _pinhole_field, _ptr_field

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
CHAIN_MIN_WEIGHT = 0.87                                      # of the chain through the real operator: the source view's weights lie
                                                             # in [0.861, 0.955], three pixels below 0.87 (depth_prior_cases)
IDS = ["%dx%d" % s for s in P.SHAPES]
FIELDS = ("D", "A", "Vi", "Vj", "match", "conf")


def _place(t, offset):
    """``t`` as a float32 GPU tensor: at the start of an allocation, or -- ``offset`` -- as a view 4 bytes into a larger one."""
    n = t.numel()
    buf = torch.empty(n + 4, dtype=F32, device=DEV)
    v = (buf[1:1 + n] if offset else buf[:n]).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 if offset else 0) and v.is_contiguous()
    return v


def _tensors(c, idx, offset):
    return tuple([_place(c[name][i], offset) for i in idx] for name in FIELDS)


def _run(c, offset=False, pairs=None, scale=1.0):
    """Forward and backward through autograd for L = sum cot_k loss_k: (loss (K,), dL/dD (K,1,H,W), dL/dA (K,1,H,W), dL/dVi (K,4,4),
    dL/dVj (K,4,4), count (K,)) on the host."""
    idx = list(range(c["K"])) if pairs is None else list(pairs)
    Ds, As, Vi, Vj, ms, cs = _tensors(c, idx, offset)
    leaves = Ds + As + Vi + Vj
    for t in leaves:
        t.requires_grad_(True)
    loss, count = correspondence_loss(Ds, As, Vi, Vj, ms, c["pin_i"][idx], c["pin_j"][idx], cs, delta=c["delta"], min_weight=P.MIN_WEIGHT,
                                      min_depth=P.MIN_DEPTH)
    assert tuple(loss.shape) == (len(idx),) == tuple(count.shape) and loss.dtype == F32 and not count.requires_grad
    grads = torch.autograd.grad(loss, leaves, (c["cot"][idx] * scale).to(DEV))
    torch.cuda.synchronize()
    n = len(idx)
    return (loss.detach().cpu(),) + tuple(torch.stack(grads[j * n:(j + 1) * n]).cpu() for j in range(4)) + (count.cpu(),)


def _c_calls(c, offset, want):
    """bags_correspondence_forward and _backward themselves, with real NULLs for what is not wanted (``want``: four flags for dL/dD,
    dL/dA, dL/dVi, dL/dVj), into buffers pre-filled with NaN; the workspace pre-filled with 0xFF."""
    idx = list(range(c["K"]))
    assert len(idx) <= L.MAX_POSE_ROWS
    Ds, As, Vi, Vj, ms, cs = _tensors(c, idx, offset)
    H, W, n = c["H"], c["W"], len(idx)
    args = L.BagsCorrespondence(H, W, n, P.MIN_WEIGHT, P.MIN_DEPTH, c["delta"], _pinhole_field([tuple(r) for r in c["pin_i"].tolist()]),
                                _pinhole_field([tuple(r) for r in c["pin_j"].tolist()]), _ptr_field(Ds), _ptr_field(As), _ptr_field(ms),
                                _ptr_field(cs), _ptr_field(Vi), _ptr_field(Vj))
    loss, count = torch.full((n,), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)
    stats = torch.full((n, L.CORRESPONDENCE_STATS), float("nan"), dtype=F64, device=DEV)
    ws = L.workspace(L.load().bags_correspondence_workspace_size(n, H, W), DEV)
    ws.fill_(255)                                            # NaN bit patterns: every partial sum that is read was written
    L.call("bags_correspondence_forward", DEV, C.byref(args), L.ptr(ws), ws.numel(), L.ptr(loss), L.ptr(count), L.ptr(stats))
    shapes = ((1, H, W), (1, H, W), (4, 4), (4, 4))
    outs = [[_place(torch.full(s, float("nan")), offset) for _ in idx] if w else None for s, w in zip(shapes, want)]
    g_loss = c["cot"].to(DEV)
    ws.fill_(255)
    views = want[2] or want[3]
    L.call("bags_correspondence_backward", DEV, C.byref(args), L.ptr(stats), L.ptr(g_loss), L.ptr(ws) if views else None, ws.numel() if views else 0,
           *(L.ptr_table(o) if o is not None else None for o in outs))
    torch.cuda.synchronize()
    return (loss.cpu(),) + tuple(torch.stack(o).cpu() if o is not None else None for o in outs) + (count.cpu(), stats.cpu())


# ---------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("delta", P.DELTAS)
@pytest.mark.parametrize("K", P.PAIRS)
@pytest.mark.parametrize("H,W", P.SHAPES, ids=IDS)
def test_values_against_float64(H, W, K, delta, offset):
    """Loss per pair, dL/dD and dL/dA per pixel, dL/dVi and dL/dVj per element within the bars of correspondence_cases.bars; the test
    prints the margins (largest error over bar; profiles/correspondence/NOTES.md has their maximum).  Invalid pixels and the fourth
    column of both matrix gradients are exact zeros (their bars are 0).  17 pairs are two launches of each kernel."""
    c = P.make_case(H, W, K, delta)
    res = _run(c, offset)
    assert all(torch.isfinite(t).all() for t in res)
    ref = P.reference(H, W, K, delta)
    assert ((res[5].double() - ref[5]).abs() <= P.EPS32 * ref[5]).all()                  # count = cnt, rounded once
    m = P.margins(H, W, K, delta, res[:5])
    print("\n%dx%d K=%d delta=%s %s: margins %s" % (H, W, K, delta, "offset" if offset else "aligned",
                                                    "  ".join("%s %.3f" % (n, x) for n, x in zip(P.NAMES, m))))
    assert all(x <= 1.0 for x in m), m                        # (a NaN fails; where a bar is 0 the value must be an exact zero)
    assert res[3][:, :, 3].abs().max() == 0 and res[4][:, :, 3].abs().max() == 0           # the fourth columns


# ---------------------------------------------------------------------------------------------------------------- bitwise
def _same(a, b, what=""):
    for x, y, name in zip(a, b, P.NAMES + ("count",)):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert torch.equal(x, y), (what, name)


@pytest.mark.parametrize("delta", P.DELTAS)
@pytest.mark.parametrize("H,W", ((17, 67), P.SEAM), ids=("17x67", "seam"))
def test_bitwise_repeats_and_a_pair_alone(H, W, delta):
    """Two runs are equal; a pair alone equals the same pair among 16; 17 pairs equal 16 + 1."""
    c = P.make_case(H, W, 16, delta)
    first, again = _run(c), _run(c)
    _same(first, again, "repeat")
    for k in (0, 6, 15):
        alone = _run(c, pairs=[k])
        assert all(torch.equal(alone[i][0], first[i][k]) for i in range(6)), k
    c17 = P.make_case(H, W, 17, delta)
    whole, head, tail = _run(c17), _run(c17, pairs=range(16)), _run(c17, pairs=[16])
    assert all(torch.equal(whole[i], torch.cat([head[i], tail[i]])) for i in range(6))


@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("delta", P.DELTAS)
def test_each_output_alone_equals_the_full_call(delta, offset):
    """Through the C entries with real NULLs; the result buffers are pre-filled with NaN and the workspace with 0xFF, so every element
    that must be written was; and without a matrix gradient the backward takes no workspace."""
    c = P.make_case(*P.SEAM, 16, delta)
    full = _c_calls(c, offset, (True, True, True, True))
    assert all(torch.isfinite(t).all() for t in full)
    for j in range(4):
        want = tuple(i == j for i in range(4))
        only = _c_calls(c, offset, want)
        assert all((only[1 + i] is None) == (not want[i]) for i in range(4))
        assert torch.equal(only[1 + j], full[1 + j]), P.NAMES[1 + j]
        assert torch.equal(only[0], full[0]) and torch.equal(only[5], full[5]) and torch.equal(only[6], full[6])
    stats = full[6]
    assert tuple(stats.shape) == (16, 2) and torch.equal(stats[:, 1].float(), full[5]) and torch.equal(stats[:, 0], 1.0 / stats[:, 1])
    _same(_run(c, offset), full[:6])                          # and autograd is those calls


# ---------------------------------------------------------------------------------------------------------------- degenerate pairs
@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("delta", P.DELTAS)
def test_degenerate_pairs(delta, offset):
    """Loss 0, count 0 and zero gradients for the pairs correspondence_cases.degenerate_case marks; every pair within the bars of the
    rule; and the eleven ordinary pairs bit for bit what a call without the five gives."""
    c = P.degenerate_case(delta)
    res = _run(c, offset)
    assert all(torch.isfinite(t).all() for t in res)
    for k in c["degenerate"]:
        assert res[0][k] == 0 and res[5][k] == 0 and all(res[i][k].abs().max() == 0 for i in (1, 2, 3, 4)), k
    r64, r32 = P.run_torch(c, F64), P.run_torch(c, F32)
    m = P.margins_of(P.bars_of(c, r64, r32), r64, res[:5])
    print("\ndegenerate delta=%s: margins %s" % (delta, m))
    assert all(x <= 1.0 for x in m), m
    keep = [k for k in range(16) if k not in c["degenerate"]]
    without = _run(c, offset, pairs=keep)
    assert all(torch.equal(without[i], res[i][keep]) for i in range(6))
    base = _run(P.make_case(17, 67, 16, delta), offset)       # ... and what the case they were put into gives
    assert all(torch.equal(base[i][keep], res[i][keep]) for i in range(6))


# ---------------------------------------------------------------------------------------------------------------- reproject_pixels
@pytest.mark.parametrize("H,W", P.SHAPES, ids=IDS)
def test_reproject_pixels(H, W):
    """proj against its statement in float64: one float32 epsilon of the terms of fx_j x_j.x / x_j.z + cx_j (their absolute values
    added) on top of what the float32 z costs the float32 statement; valid identical where the projections stay 1e-3 px clear of the
    border of the target image (the size is chosen so that they do)."""
    c = P.make_case(H, W, 2, 1.0)
    for k in range(2):
        a = (c["D"][k], c["A"][k], c["Vi"][k], c["Vj"][k], c["pin_i"][k], c["pin_j"][k])
        kw = dict(min_weight=P.MIN_WEIGHT, min_depth=P.MIN_DEPTH)
        p64, _ = reproject_pixels_torch(a[0].double(), a[1].double(), *a[2:], (1 << 20, 1 << 20), **kw)
        size = None
        for cand in ((H, W), (H + 3, W - 2), (2 * H, 3 * W), (max(1, H // 2), max(1, W // 2))):       # one whose border nothing comes near
            edge = torch.stack([p64[0] + 0.5, p64[0] - (cand[1] - 0.5), p64[1] + 0.5, p64[1] - (cand[0] - 0.5)]).abs().min().item()
            if cand[0] >= 1 and cand[1] >= 1 and edge >= 1e-3:
                size = cand
                break
        assert size is not None
        p64, ok64 = reproject_pixels_torch(a[0].double(), a[1].double(), *a[2:], size, **kw)
        p32, ok32 = reproject_pixels_torch(*a, size, **kw)
        proj, valid = reproject_pixels(_place(a[0], bool(k)), _place(a[1], bool(k)), a[2].to(DEV), a[3].to(DEV), a[4], a[5], size, **kw)
        torch.cuda.synchronize()
        assert proj.dtype == F32 and tuple(proj.shape) == (2, H, W) and valid.dtype == torch.bool and tuple(valid.shape) == (H, W)
        assert torch.equal(ok32, ok64) and torch.equal(valid.cpu(), ok64)
        q = P._pieces(c)
        xj, pj = q["xi"][k].reshape(-1, 3) @ q["M"][k] + q["c"][k], c["pin_j"][k]
        terms = torch.stack([(pj[0] * xj[:, 0] / xj[:, 2]).abs() + abs(pj[2]), (pj[1] * xj[:, 1] / xj[:, 2]).abs() + abs(pj[3])]).view(2, H, W)
        geometric = (p64 != 0).any(0)
        bar = torch.where(geometric, (p32.double() - p64).abs() + P.EPS32 * terms, torch.zeros_like(terms))
        err = (proj.cpu().double() - p64).abs()
        assert (err <= bar).all(), float((err / bar.clamp_min(1e-300)).max())
        if H >= 7:
            assert ok64.any() and (~ok64).any()


# ---------------------------------------------------------------------------------------------------------------- autograd
def test_no_grad_keeps_nothing_and_an_in_place_write_raises():
    c = P.make_case(17, 67, 2, 1.0)
    Ds, As, Vi, Vj, ms, cs = _tensors(c, [0, 1], False)
    pi, pj = c["pin_i"], c["pin_j"]
    loss, count = correspondence_loss(Ds, As, Vi, Vj, ms, pi, pj, cs)
    assert loss.grad_fn is None and not loss.requires_grad and count.grad_fn is None             # constant inputs
    del loss, count
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    for t in Ds + As + Vi + Vj:
        t.requires_grad_(True)
    with torch.no_grad():
        loss, count = correspondence_loss(Ds, As, Vi, Vj, ms, pi, pj, cs)
    assert loss.grad_fn is None and not loss.requires_grad
    del loss, count
    assert torch.cuda.memory_allocated() == held              # nothing was saved
    loss, count = correspondence_loss(Ds, As, Vi, Vj, ms, pi, pj, cs)
    assert loss.grad_fn is not None and type(loss.grad_fn).__name__.startswith("_Correspondence") and not count.requires_grad
    only = correspondence_loss(Ds[0], As[0].detach(), Vi[0].detach(), Vj[0], ms[0], pi[0], pj[0])[0]        # one pair, no conf
    only.sum().backward()
    assert Ds[0].grad is not None and Vj[0].grad is not None and As[0].grad is None and Vi[0].grad is None
    # a source view in two pairs: autograd adds its gradients
    D = Ds[1].detach().clone().requires_grad_(True)
    two = correspondence_loss([D, D], [As[1].detach()] * 2, [Vi[1].detach()] * 2, [Vj[1].detach(), Vj[0].detach()], [ms[1], ms[0]], pi[1], pj[1])[0]
    parts = [torch.autograd.grad(two[i], D, retain_graph=True)[0] for i in range(2)]
    two.sum().backward()
    assert torch.equal(D.grad, parts[0] + parts[1]) and parts[0].abs().max() > 0 and parts[1].abs().max() > 0
    # the adjoint re-reads the maps: an in-place write between forward and backward raises
    D2 = Ds[1].detach().clone().requires_grad_(True)
    D2w = D2 * 1.0
    loss = correspondence_loss(D2w, As[1].detach(), Vi[1].detach(), Vj[1].detach(), ms[1], pi[1], pj[1])[0]
    D2w.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.sum().backward()
    with pytest.raises(RuntimeError, match="AMD GPU"):
        correspondence_loss(c["D"][0], As[0], Vi[0], Vj[0], ms[0], pi[0], pj[0])             # a host map into the HIP path: refused
    with pytest.raises(TypeError, match=r"\.float\(\)"):
        correspondence_loss(Ds[0], As[0], Vi[0], Vj[0], ms[0], pi[0], pj[0], cs[0] > 0)
    with pytest.raises(ValueError, match="GPU tensor"):
        correspondence_loss(Ds[0], As[0], Vi[0], Vj[0], ms[0], pi[0].to(DEV), pj[0])
    with pytest.raises(ValueError, match="GPU tensor"):
        reproject_pixels(Ds[0], As[0], Vi[0], Vj[0], pi[0], pj[0].to(DEV), (17, 67))
    with pytest.raises(TypeError, match="float32"):
        correspondence_loss(Ds[0], As[0], Vi[0].double(), Vj[0], ms[0], pi[0], pj[0])


# ---------------------------------------------------------------------------------------------------------------- chain
def test_chain_with_the_real_operator():
    """render_views(depth_weights_grad=True) of two PoseCameras -> correspondence_loss on the pair (0 -> 1) with the cameras' own view
    matrices -> backward reaches xyz and both cameras' pose leaves.  The matches are reproject_pixels at the true poses; the target
    pose is then perturbed, so the loss is positive.  The gradients with respect to the two maps and the two view matrices are held
    to the float64 statement run on those maps, within the bars of the rule (correspondence_cases.bars_of)."""
    from bags_raster import GaussianBag, PipelineParams, render_views
    from bags_raster.synth import look_at_origin_camera, so3_exp, synth_scene
    H = W = 32
    bag = GaussianBag.from_activated(synth_scene(24, 5, 3.0, 1), 1, device=DEV)
    cams = [look_at_origin_camera(W, H, dist=3.0, device=DEV),
            look_at_origin_camera(W, H, dist=3.0, device=DEV, R=so3_exp(torch.tensor((0.03, -0.05, 0.02))), T=torch.tensor((0.15, -0.1, 3.05)))]
    pins = [pinhole_of(cam.get_intrinsic(), H, W) for cam in cams]
    bg, pipe = torch.zeros(3, device=DEV), PipelineParams()

    with torch.no_grad():
        pk = render_views(cams, bag, pipe, bg, 0.0, None)[0]
        views = [cam.get_matrices()[0] for cam in cams]
        match, covisible = reproject_pixels(pk["depth"], pk["weights"], views[0], views[1], pins[0], pins[1], (H, W), min_weight=CHAIN_MIN_WEIGHT)
        gap = (pk["weights"] - CHAIN_MIN_WEIGHT).abs().min().item()
        zero = correspondence_loss(pk["depth"], pk["weights"], views[0], views[1], match, pins[0], pins[1], min_weight=CHAIN_MIN_WEIGHT)
        cams[1].delta_translation.add_(torch.tensor((0.02, -0.015, 0.01), device=DEV).view(3, 1))       # the target pose, perturbed
        cams[1].delta_quaternion.add_(torch.tensor((0.0, 0.004, -0.003, 0.002), device=DEV))
    print("\nchain: |weights - min_weight| >= %.3g, covisible share %.3f, loss at the true poses %.3g" % (gap, covisible.float().mean().item(), zero[0].item()))
    assert gap >= 5e-4 and covisible.float().mean().item() >= 0.25 and zero[0].item() <= 1e-6 and zero[1].item() >= 0.25 * H * W
    conf = torch.where(covisible, 1.0, 0.0) * (0.25 + 0.75 * torch.rand(H, W, generator=torch.Generator().manual_seed(31))).to(DEV)

    pkgs = render_views(cams, bag, pipe, bg, 0.0, None, depth_weights_grad=True)
    depth, weights = pkgs[0]["depth"], pkgs[0]["weights"]
    views = [cam.get_matrices()[0] for cam in cams]
    assert depth.requires_grad and weights.requires_grad and all(v.requires_grad for v in views)
    for t in (depth, weights, *views):
        t.retain_grad()
    loss, count = correspondence_loss(depth, weights, views[0], views[1], match, pins[0], pins[1], conf, delta=1.0, min_weight=CHAIN_MIN_WEIGHT)
    assert loss.item() > 0 and count.item() > 0
    loss.sum().backward()
    torch.cuda.synchronize()
    for name, t in (("xyz", bag._xyz), ("dq0", cams[0].delta_quaternion), ("dt0", cams[0].delta_translation), ("dq1", cams[1].delta_quaternion),
                    ("dt1", cams[1].delta_translation)):
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().max().item() > 0, name
    # the float64 statement on those maps
    c = dict(H=H, W=W, K=1, delta=1.0, D=depth.detach().cpu()[None], A=weights.detach().cpu()[None], conf=conf.cpu()[None], match=match.cpu()[None],
             Vi=views[0].detach().cpu()[None], Vj=views[1].detach().cpu()[None], pin_i=torch.tensor(pins[:1], dtype=F64),
             pin_j=torch.tensor(pins[1:], dtype=F64), cot=torch.ones(1), degenerate=(), min_weight=CHAIN_MIN_WEIGHT)
    r64, r32 = P.run_torch(c, F64), P.run_torch(c, F32)
    bar = P.bars_of(c, r64, r32)
    got = (loss.detach().cpu(), depth.grad.cpu()[None], weights.grad.cpu()[None], views[0].grad.cpu()[None], views[1].grad.cpu()[None])
    m = P.margins_of(bar, r64, got)
    print("chain margins: %s" % "  ".join("%s %.3f" % (n, x) for n, x in zip(P.NAMES, m)))
    assert abs(count.item() - r64[5].item()) <= P.EPS32 * r64[5].item() and r64[0].item() > 0
    assert all(x <= 1.0 for x in m), m
