"""GPU checks of the warping loss: bags_raster.warp_loss / warp_image (csrc/warp.hip) against warp_loss_torch in float64 on the cases
of tests/warp_cases.py, held to that module's bars; the bitwise properties of its sums and its optional outputs; the degenerate
pairs; warp_image; the autograd behaviour; and the chain render_views -> warp_loss -> backward."""
import ctypes as C

import pytest
import torch

import warp_cases as P
from bags_raster import _lib as L, pinhole_of, warp_image, warp_image_torch, warp_loss
from bags_raster.warp import _pinhole_field, _ptr_field

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
CHAIN_MIN_WEIGHT = 0.87                                      # of the chain through the real operator: the rendered weights of both views
                                                             # stay clear of it (the test asserts the gap)
IDS = ["%dx%d" % s for s in P.SHAPES]
FIELDS = ("D", "A", "Vi", "Vj", "color", "image", "conf", "D_dst", "A_dst")


def _place(t, offset):
    """``t`` as a float32 GPU tensor: at the start of an allocation, or -- ``offset`` -- as a view 4 bytes into a larger one."""
    n = t.numel()
    buf = torch.empty(n + 4, dtype=F32, device=DEV)
    v = (buf[1:1 + n] if offset else buf[:n]).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 if offset else 0) and v.is_contiguous()
    return v


def _tensors(c, idx, offset):
    """The nine tensor groups of a call; a pair without target maps has None in the last two."""
    groups = [[_place(c[name][i], offset) for i in idx] for name in FIELDS[:7]]
    groups += [[_place(c[name][i], offset) if bool(c["has_dst"][i]) else None for i in idx] for name in FIELDS[7:]]
    return groups


def _run(c, offset=False, pairs=None, scale=1.0):
    """Forward and backward through autograd for L = sum cot_k loss_k: (loss (K,), dL/dD (K,1,H,W), dL/dA (K,1,H,W), dL/dVi (K,4,4),
    dL/dVj (K,4,4), count (K,)) on the host."""
    idx = list(range(c["K"])) if pairs is None else list(pairs)
    Ds, As, Vi, Vj, cols, imgs, cs, Dt, At = _tensors(c, idx, offset)
    leaves = Ds + As + Vi + Vj
    for t in leaves:
        t.requires_grad_(True)
    loss, count = warp_loss(Ds, As, Vi, Vj, cols, imgs, c["pin_i"][idx], c["pin_j"][idx], cs, Dt, At, eps=c["eps"], occlusion=P.OCCLUSION,
                            min_weight=P.MIN_WEIGHT, min_depth=P.MIN_DEPTH)
    assert tuple(loss.shape) == (len(idx),) == tuple(count.shape) and loss.dtype == F32 and not count.requires_grad
    grads = torch.autograd.grad(loss, leaves, (c["cot"][idx] * scale).to(DEV))
    torch.cuda.synchronize()
    n = len(idx)
    return (loss.detach().cpu(),) + tuple(torch.stack(grads[j * n:(j + 1) * n]).cpu() for j in range(4)) + (count.cpu(),)


def _args(c, groups, n):
    Ds, As, Vi, Vj, cols, imgs, cs, Dt, At = groups
    return L.BagsWarp(c["H"], c["W"], n, P.MIN_WEIGHT, P.MIN_DEPTH, c["C"], c["Hd"], c["Wd"], 0, c["eps"], P.OCCLUSION,
                      _pinhole_field([tuple(r) for r in c["pin_i"].tolist()]), _pinhole_field([tuple(r) for r in c["pin_j"].tolist()]),
                      _ptr_field(Ds), _ptr_field(As), _ptr_field(cs), _ptr_field(Vi), _ptr_field(Vj), _ptr_field(cols), _ptr_field(imgs),
                      _ptr_field(Dt), _ptr_field(At))


def _c_calls(c, offset, want):
    """bags_warp_forward and _backward themselves, with real NULLs for what is not wanted (``want``: four flags for dL/dD, dL/dA, dL/dVi,
    dL/dVj), into buffers pre-filled with NaN; the workspace pre-filled with 0xFF."""
    idx = list(range(c["K"]))
    assert len(idx) <= L.MAX_POSE_ROWS
    groups = _tensors(c, idx, offset)
    H, W, n = c["H"], c["W"], len(idx)
    args = _args(c, groups, n)
    loss, count = torch.full((n,), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)
    stats = torch.full((n, L.CORRESPONDENCE_STATS), float("nan"), dtype=F64, device=DEV)
    ws = L.workspace(L.load().bags_warp_workspace_size(n, H, W), DEV)
    ws.fill_(255)                                            # NaN bit patterns: every partial sum that is read was written
    L.call("bags_warp_forward", DEV, C.byref(args), L.ptr(ws), ws.numel(), L.ptr(loss), L.ptr(count), L.ptr(stats))
    shapes = ((1, H, W), (1, H, W), (4, 4), (4, 4))
    outs = [[_place(torch.full(s, float("nan")), offset) for _ in idx] if w else None for s, w in zip(shapes, want)]
    g_loss = c["cot"].to(DEV)
    ws.fill_(255)
    views = want[2] or want[3]
    L.call("bags_warp_backward", DEV, C.byref(args), L.ptr(stats), L.ptr(g_loss), L.ptr(ws) if views else None, ws.numel() if views else 0,
           *(L.ptr_table(o) if o is not None else None for o in outs))
    torch.cuda.synchronize()
    return (loss.cpu(),) + tuple(torch.stack(o).cpu() if o is not None else None for o in outs) + (count.cpu(), stats.cpu())


# ---------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("eps", P.EPSES)
@pytest.mark.parametrize("channels", P.CHANNELS)
@pytest.mark.parametrize("K", P.PAIRS)
@pytest.mark.parametrize("H,W", P.SHAPES, ids=IDS)
def test_values_against_float64(H, W, K, channels, eps, offset):
    """Loss per pair, dL/dD and dL/dA per pixel, dL/dVi and dL/dVj per element within the bars of warp_cases.bars; the test prints the
    margins (largest error over bar; profiles/warp/NOTES.md has their maximum).  Invalid pixels and the fourth column of both matrix
    gradients are exact zeros (their bars are 0).  17 pairs are two launches of each kernel."""
    c = P.make_case(H, W, K, channels, eps)
    res = _run(c, offset)
    assert all(torch.isfinite(t).all() for t in res)
    ref = P.reference(H, W, K, channels, eps)
    assert ((res[5].double() - ref[5]).abs() <= P.EPS32 * ref[5]).all()                  # count = cnt, rounded once
    m = P.margins(H, W, K, channels, eps, res[:5])
    print("\n%dx%d K=%d C=%d eps=%s %s: margins %s" % (H, W, K, channels, eps, "offset" if offset else "aligned",
                                                       "  ".join("%s %.3f" % (n, x) for n, x in zip(P.NAMES, m))))
    assert all(x <= 1.0 for x in m), m                        # (a NaN fails; where a bar is 0 the value must be an exact zero)
    assert res[3][:, :, 3].abs().max() == 0 and res[4][:, :, 3].abs().max() == 0           # the fourth columns


# ---------------------------------------------------------------------------------------------------------------- bitwise
def _same(a, b, what=""):
    for x, y, name in zip(a, b, P.NAMES + ("count",)):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert torch.equal(x, y), (what, name)


@pytest.mark.parametrize("channels", P.CHANNELS)
@pytest.mark.parametrize("H,W", ((17, 67), P.SEAM), ids=("17x67", "seam"))
def test_bitwise_repeats_and_a_pair_alone(H, W, channels):
    """Two runs are equal; a pair alone equals the same pair among 16 (pair 1 has no target maps, its neighbours have); 17 pairs equal
    16 + 1."""
    c = P.make_case(H, W, 16, channels, 1e-3)
    first, again = _run(c), _run(c)
    _same(first, again, "repeat")
    for k in (0, 1, 6, 15):
        alone = _run(c, pairs=[k])
        assert all(torch.equal(alone[i][0], first[i][k]) for i in range(6)), k
    c17 = P.make_case(H, W, 17, channels, 1e-3)
    whole, head, tail = _run(c17), _run(c17, pairs=range(16)), _run(c17, pairs=[16])
    assert all(torch.equal(whole[i], torch.cat([head[i], tail[i]])) for i in range(6))


def test_a_pair_with_target_maps_keeps_its_bits_next_to_pairs_without():
    """The occlusion test is per pair: the pairs with target maps give the same bits whether their neighbours have target maps or
    not, and a pair gives what it gives without the test exactly where its maps are withheld."""
    c = P.make_case(*P.SEAM, 16, 3, 1e-3)
    full = _run(c)
    bare = dict(c, has_dst=torch.zeros(16, dtype=torch.bool))
    none = _run(bare)
    mixed = dict(c, has_dst=torch.tensor([k % 2 == 0 for k in range(16)]))
    res = _run(mixed)
    for k in range(16):
        src = full if (k % 2 == 0 and bool(c["has_dst"][k])) else none
        assert all(torch.equal(res[i][k], src[i][k]) for i in range(6)), k
    assert not torch.equal(full[0][0], none[0][0])            # the test does take pixels out


@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("channels", P.CHANNELS)
def test_each_output_alone_equals_the_full_call(channels, offset):
    """Through the C entries with real NULLs; the result buffers are pre-filled with NaN and the workspace with 0xFF, so every element
    that must be written was; and without a matrix gradient the backward takes no workspace."""
    c = P.make_case(*P.SEAM, 16, channels, 0.1)
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
@pytest.mark.parametrize("eps", P.EPSES)
@pytest.mark.parametrize("channels", P.CHANNELS)
def test_degenerate_pairs(channels, eps, offset):
    """Loss 0, count 0 and zero gradients for the six pairs warp_cases.degenerate_case marks; every pair within the bars of the rule;
    and the ten ordinary pairs bit for bit what a call without the six gives."""
    c = P.degenerate_case(channels, eps)
    res = _run(c, offset)
    assert all(torch.isfinite(t).all() for t in res)
    for k in c["degenerate"]:
        assert res[0][k] == 0 and res[5][k] == 0 and all(res[i][k].abs().max() == 0 for i in (1, 2, 3, 4)), k
    r64, r32 = P.run_torch(c, F64), P.run_torch(c, F32)
    m = P.margins_of(P.bars_of(c, r64, r32), r64, res[:5])
    print("\ndegenerate C=%d eps=%s: margins %s" % (channels, eps, m))
    assert all(x <= 1.0 for x in m), m
    keep = [k for k in range(16) if k not in c["degenerate"]]
    without = _run(c, offset, pairs=keep)
    assert all(torch.equal(without[i], res[i][keep]) for i in range(6))
    base = _run(P.make_case(17, 67, 16, channels, eps), offset)       # ... and what the case they were put into gives
    assert all(torch.equal(base[i][keep], res[i][keep]) for i in range(6))


# ---------------------------------------------------------------------------------------------------------------- warp_image
@pytest.mark.parametrize("channels", P.CHANNELS)
@pytest.mark.parametrize("H,W", P.SHAPES, ids=IDS)
def test_warp_image(H, W, channels):
    """valid identical to the float64 statement's (the generator's guards keep every pixel with conf > 0 clear of a decision; the
    guarded pixels, whose decision float32 may take the other way, are left out of the comparison); the colours within one float32
    epsilon of the sum of |weight x tap| on top of what the float32 z costs the float32 statement."""
    c = P.make_case(H, W, 2, channels, 1e-3)
    q = P._pieces(c)
    for k in range(2):
        maps = (c["D_dst"][k], c["A_dst"][k]) if bool(c["has_dst"][k]) else (None, None)
        a = (c["D"][k], c["A"][k], c["Vi"][k], c["Vj"][k], c["image"][k], c["pin_i"][k], c["pin_j"][k]) + maps
        kw = dict(occlusion=P.OCCLUSION, min_weight=P.MIN_WEIGHT, min_depth=P.MIN_DEPTH)
        w64, ok64 = warp_image_torch(*(t.double() if torch.is_tensor(t) else t for t in a), **kw)
        w32, ok32 = warp_image_torch(*a, **kw)
        dev = [None if t is None else _place(t, bool(k)) for t in (a[0], a[1], a[2], a[3], a[4], a[7], a[8])]
        out, valid = warp_image(dev[0], dev[1], dev[2], dev[3], dev[4], a[5], a[6], dev[5], dev[6], **kw)
        torch.cuda.synchronize()
        assert out.dtype == F32 and tuple(out.shape) == (channels, H, W) and valid.dtype == torch.bool and tuple(valid.shape) == (H, W)
        clear = ~c["guarded"][k]
        assert torch.equal(ok32[clear], ok64[clear]) and torch.equal(valid.cpu()[clear], ok64[clear])
        assert ok64[clear].any() and (H * W < 200 or (~ok64[clear]).any())
        t00, t01, t10, t11 = (t[k].abs() for t in q["taps"])          # zero where the pixel is not valid for the loss
        ax, ay = q["ax"][k], q["ay"][k]
        terms = (1 - ay) * ((1 - ax) * t00 + ax * t01) + ay * ((1 - ax) * t10 + ax * t11)
        both = (clear & ok64 & q["valid"][k])[None].expand_as(terms)
        bar = (w32.double() - w64).abs() + P.EPS32 * terms
        err = (out.cpu().double() - w64).abs()
        assert (err[both] <= bar[both]).all(), float((err[both] / bar[both].clamp_min(1e-300)).max())
        assert out.cpu()[:, ~valid.cpu()].abs().max() == 0 if (~valid).any() else True


# ---------------------------------------------------------------------------------------------------------------- autograd
def test_no_grad_keeps_nothing_and_an_in_place_write_raises():
    c = P.make_case(17, 67, 2, 3, 1e-3)
    Ds, As, Vi, Vj, cols, imgs, cs, Dt, At = _tensors(c, [0, 1], False)
    pi, pj = c["pin_i"], c["pin_j"]
    loss, count = warp_loss(Ds, As, Vi, Vj, cols, imgs, pi, pj, cs, Dt, At)
    assert loss.grad_fn is None and not loss.requires_grad and count.grad_fn is None             # constant inputs
    del loss, count
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    for t in Ds + As + Vi + Vj:
        t.requires_grad_(True)
    with torch.no_grad():
        loss, count = warp_loss(Ds, As, Vi, Vj, cols, imgs, pi, pj, cs, Dt, At)
    assert loss.grad_fn is None and not loss.requires_grad
    del loss, count
    assert torch.cuda.memory_allocated() == held              # nothing was saved
    loss, count = warp_loss(Ds, As, Vi, Vj, cols, imgs, pi, pj, cs, Dt, At)
    assert loss.grad_fn is not None and type(loss.grad_fn).__name__.startswith("_Warp") and not count.requires_grad
    only = warp_loss(Ds[0], As[0].detach(), Vi[0].detach(), Vj[0], cols[0], imgs[0], pi[0], pj[0])[0]        # one pair, no conf, no target maps
    only.sum().backward()
    assert Ds[0].grad is not None and Vj[0].grad is not None and As[0].grad is None and Vi[0].grad is None
    # an image that carries a gradient gets none: it is constant data
    img = imgs[0].clone().requires_grad_(True)
    warp_loss(Ds[0], As[0], Vi[0], Vj[0], cols[0], img, pi[0], pj[0])[0].sum().backward()
    assert img.grad is None
    # a source view in two pairs: autograd adds its gradients
    D = Ds[1].detach().clone().requires_grad_(True)
    two = warp_loss([D, D], [As[1].detach()] * 2, [Vi[1].detach()] * 2, [Vj[1].detach()] * 2, [cols[1], cols[1] + 0.05], [imgs[1]] * 2, pi[1], pj[1])[0]
    parts = [torch.autograd.grad(two[i], D, retain_graph=True)[0] for i in range(2)]
    two.sum().backward()
    assert torch.equal(D.grad, parts[0] + parts[1]) and parts[0].abs().max() > 0 and parts[1].abs().max() > 0
    # the adjoint re-reads the maps: an in-place write between forward and backward raises
    D2 = Ds[1].detach().clone().requires_grad_(True)
    D2w = D2 * 1.0
    loss = warp_loss(D2w, As[1].detach(), Vi[1].detach(), Vj[1].detach(), cols[1], imgs[1], pi[1], pj[1])[0]
    D2w.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.sum().backward()
    with pytest.raises(RuntimeError, match="AMD GPU"):
        warp_loss(c["D"][0], As[0], Vi[0], Vj[0], cols[0], imgs[0], pi[0], pj[0])             # a host map into the HIP path: refused
    with pytest.raises(RuntimeError, match="AMD GPU"):
        warp_loss(Ds[0], As[0], Vi[0], Vj[0], cols[0], c["image"][0], pi[0], pj[0])           # ... and a host image
    with pytest.raises(TypeError, match=r"\.float\(\)"):
        warp_loss(Ds[0], As[0], Vi[0], Vj[0], cols[0], imgs[0], pi[0], pj[0], cs[0] > 0)
    with pytest.raises(ValueError, match="GPU tensor"):
        warp_loss(Ds[0], As[0], Vi[0], Vj[0], cols[0], imgs[0], pi[0].to(DEV), pj[0])
    with pytest.raises(ValueError, match="GPU tensor"):
        warp_image(Ds[0], As[0], Vi[0], Vj[0], imgs[0], pi[0], pj[0].to(DEV))
    with pytest.raises(TypeError, match="float32"):
        warp_loss(Ds[0], As[0], Vi[0].double(), Vj[0], cols[0], imgs[0], pi[0], pj[0])
    with pytest.raises(TypeError, match="float32"):
        warp_loss(Ds[0], As[0], Vi[0], Vj[0], cols[0], imgs[0].double(), pi[0], pj[0])


# ---------------------------------------------------------------------------------------------------------------- chain
def test_chain_with_the_real_operator():
    """render_views(depth_weights_grad=True) of two PoseCameras at 32 x 32 -> warp_loss on the pair (0 -> 1) with the cameras' own view
    matrices, the two rendered images (detached) as color_src and image_dst and the second view's maps as target maps -> backward
    reaches xyz and both cameras' pose leaves.  The target pose is perturbed after the images were rendered, so the loss is positive.
    The gradients with respect to the two maps and the two view matrices are held to the float64 statement run on those maps, within
    the bars of the rule (warp_cases.bars_of)."""
    from bags_raster import GaussianBag, PipelineParams, render_views
    from bags_raster.synth import look_at_origin_camera, so3_exp, synth_scene
    H = W = 32
    bag = GaussianBag.from_activated(synth_scene(24, 5, 3.0, 1), 1, device=DEV)
    cams = [look_at_origin_camera(W, H, dist=3.0, device=DEV),
            look_at_origin_camera(W, H, dist=3.0, device=DEV, R=so3_exp(torch.tensor((0.03, -0.05, 0.02))), T=torch.tensor((0.15, -0.1, 3.05)))]
    pins = [pinhole_of(cam.get_intrinsic(), H, W) for cam in cams]
    bg, pipe = torch.zeros(3, device=DEV), PipelineParams()

    with torch.no_grad():
        pk = render_views(cams, bag, pipe, bg, 0.0, None)
        images = [p["render"].detach().contiguous() for p in pk]
        target = (pk[1]["depth"].detach().contiguous(), pk[1]["weights"].detach().contiguous())
        views = [cam.get_matrices()[0] for cam in cams]
        gap = min((p["weights"] - CHAIN_MIN_WEIGHT).abs().min().item() for p in pk)
        warped, covisible = warp_image(pk[0]["depth"], pk[0]["weights"], views[0], views[1], images[1], pins[0], pins[1], *target,
                                       min_weight=CHAIN_MIN_WEIGHT)
        cams[1].delta_translation.add_(torch.tensor((0.02, -0.015, 0.01), device=DEV).view(3, 1))       # the target pose, perturbed
        cams[1].delta_quaternion.add_(torch.tensor((0.0, 0.004, -0.003, 0.002), device=DEV))
    print("\nchain: |weights - min_weight| >= %.3g, covisible share %.3f" % (gap, covisible.float().mean().item()))
    assert gap >= 5e-4 and covisible.float().mean().item() >= 0.25

    pkgs = render_views(cams, bag, pipe, bg, 0.0, None, depth_weights_grad=True)
    depth, weights = pkgs[0]["depth"], pkgs[0]["weights"]
    views = [cam.get_matrices()[0] for cam in cams]
    assert depth.requires_grad and weights.requires_grad and all(v.requires_grad for v in views)
    for t in (depth, weights, *views):
        t.retain_grad()
    # the case of the float64 statement on those maps; its confidence is 0 where that statement lies within 1e-3 of a decision, as in
    # every case of warp_cases (the guards), and fractional elsewhere
    conf = 0.25 + 0.75 * torch.rand(H, W, generator=torch.Generator().manual_seed(31))
    c = dict(H=H, W=W, K=1, Hd=H, Wd=W, C=3, eps=1e-3, D=depth.detach().cpu()[None], A=weights.detach().cpu()[None], conf=conf[None],
             color=images[0].cpu()[None], image=images[1].cpu()[None], D_dst=target[0].cpu()[None], A_dst=target[1].cpu()[None],
             has_dst=torch.ones(1, dtype=torch.bool), Vi=views[0].detach().cpu()[None], Vj=views[1].detach().cpu()[None],
             pin_i=torch.tensor(pins[:1], dtype=F64), pin_j=torch.tensor(pins[1:], dtype=F64), cot=torch.ones(1), degenerate=(),
             min_weight=CHAIN_MIN_WEIGHT)
    guard = P.guard_mask(c)[0]
    c["conf"] = torch.where(guard, torch.zeros_like(c["conf"]), c["conf"])
    print("chain: %d of %d pixels within 1e-3 of a decision" % (int(guard.sum()), H * W))
    assert guard.double().mean().item() <= 0.03
    loss, count = warp_loss(depth, weights, views[0], views[1], images[0], images[1], pins[0], pins[1], c["conf"][0].to(DEV), *target, eps=1e-3,
                            occlusion=P.OCCLUSION, min_weight=CHAIN_MIN_WEIGHT, min_depth=P.MIN_DEPTH)
    assert loss.item() > 0 and count.item() >= 0.25 * H * W
    loss.sum().backward()
    torch.cuda.synchronize()
    for name, t in (("xyz", bag._xyz), ("dq0", cams[0].delta_quaternion), ("dt0", cams[0].delta_translation), ("dq1", cams[1].delta_quaternion),
                    ("dt1", cams[1].delta_translation)):
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().max().item() > 0, name
    r64, r32 = P.run_torch(c, F64), P.run_torch(c, F32)
    bar = P.bars_of(c, r64, r32)
    got = (loss.detach().cpu(), depth.grad.cpu()[None], weights.grad.cpu()[None], views[0].grad.cpu()[None], views[1].grad.cpu()[None])
    m = P.margins_of(bar, r64, got)
    print("chain margins: %s" % "  ".join("%s %.3f" % (n, x) for n, x in zip(P.NAMES, m)))
    assert abs(r32[5].item() - r64[5].item()) <= P.EPS32 * r64[5].item()                  # the two statements took the same decisions
    assert abs(count.item() - r64[5].item()) <= P.EPS32 * r64[5].item() and r64[0].item() > 0
    assert all(x <= 1.0 for x in m), m
