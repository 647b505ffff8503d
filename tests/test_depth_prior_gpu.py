"""GPU checks of the depth prior: bags_raster.depth_prior_loss / DepthPriorBank (csrc/depth_prior.hip) against
depth_prior_loss_torch in float64 on the cases of tests/depth_prior_cases.py, held to that module's bars; the bitwise properties of
its two paths, its optional outputs and its sums; the degenerate views; and the chain rasterizer -> depth_prior_loss -> backward."""
import ctypes as C

import pytest
import torch

import depth_prior_cases as P
from bags_raster import DepthPriorBank, _lib as L, depth_prior_loss, depth_prior_loss_torch
from bags_raster.depth_prior import MODES, SPACES, _ptr_field
from bags_raster.pose_bank import _row_table

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
COMBOS = [(m, s) for m in P.MODES for s in P.SPACES]
COMBO_IDS = ["%s-%s" % ms for ms in COMBOS]
VECTOR_SHAPES = tuple(s for s in P.SHAPES if s[1] % 4 == 0)          # (16, 64) and the strided shape
NAMES = ("loss", "dL/dD", "dL/dA", "dL/dtable")


def _place(t, offset):
    """``t`` as a float32 GPU tensor: at the start of an allocation (16-byte aligned), or -- ``offset`` -- as a view 4 bytes into
    a larger one, which no float4 access may touch: the scalar path."""
    n = t.numel()
    buf = torch.empty(n + 4, dtype=F32, device=DEV)
    v = (buf[1:1 + n] if offset else buf[:n]).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 if offset else 0) and v.is_contiguous()
    return v


def _maps(c, idx, offset):
    return ([_place(c["D"][i], offset) for i in idx], [_place(c["A"][i], offset) for i in idx],
            [_place(c["prior"][i], offset) for i in idx], [_place(c["mask"][i], offset) for i in idx])


def _run(c, offset=False, views=None, scale=1.0):
    """Forward and backward through autograd for L = sum cot_v loss_v: (loss (V,), dL/dD (V,1,H,W), dL/dA (V,1,H,W), dL/dtable (N,2) or
    None, count (V,)) on the host."""
    idx = list(range(c["V"])) if views is None else list(views)
    Ds, As, ps, ms = _maps(c, idx, offset)
    for t in Ds + As:
        t.requires_grad_(True)
    kw, leaves = {}, Ds + As
    if c["mode"] == "l1":
        table = c["table"].to(DEV).requires_grad_(True)
        kw, leaves = dict(table=table, rows=[c["rows"][i] for i in idx]), leaves + [table]
    loss, count = depth_prior_loss(Ds, As, ps, ms, mode=c["mode"], space=c["space"], min_weight=P.MIN_WEIGHT, **kw)
    assert tuple(loss.shape) == (len(idx),) == tuple(count.shape) and loss.dtype == F32 and not count.requires_grad
    grads = torch.autograd.grad(loss, leaves, (c["cot"][idx] * scale).to(DEV))
    torch.cuda.synchronize()
    n = len(idx)
    return (loss.detach().cpu(), torch.stack(grads[:n]).cpu(), torch.stack(grads[n:2 * n]).cpu(), grads[2 * n].cpu() if kw else None,
            count.cpu())


def _got(c, res, views=None):
    """What the margins compare: the table gradient as the listed rows, in list order; every other row is checked to be zero."""
    idx = list(range(c["V"])) if views is None else list(views)
    g_table = res[3]
    if g_table is None:
        return res[:3] + (None,)
    rows = [c["rows"][i] for i in idx]
    other = [r for r in range(P.N) if r not in rows]
    assert tuple(g_table.shape) == (P.N, 2) and torch.isfinite(g_table).all()
    assert not other or g_table[other].abs().max().item() == 0.0
    return res[:3] + (g_table[rows],)


def _struct(c, idx, maps, table):
    Ds, As, ps, ms = maps
    return L.BagsDepthPrior(MODES[c["mode"]], SPACES[c["space"]], c["H"], c["W"], P.MIN_WEIGHT, len(idx), P.N if table is not None else 0, 0,
                            L.ptr(table), _row_table([c["rows"][i] for i in idx]), _ptr_field(Ds), _ptr_field(As), _ptr_field(ps), _ptr_field(ms))


def _c_calls(c, offset, want_depth, want_weights, want_table):
    """bags_depth_prior_forward and _backward themselves, with real NULLs for what is not wanted, into buffers pre-filled with NaN."""
    idx = list(range(c["V"]))
    assert len(idx) <= L.MAX_POSE_ROWS
    maps = _maps(c, idx, offset)
    table = c["table"].to(DEV) if c["mode"] == "l1" else None
    H, W, n = c["H"], c["W"], len(idx)
    args = _struct(c, idx, maps, table)
    loss, count = torch.full((n,), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)
    stats = torch.full((n, L.DEPTH_PRIOR_STATS), float("nan"), dtype=F64, device=DEV)
    ws = L.workspace(L.load().bags_depth_prior_workspace_size(n, H, W), DEV)
    ws.fill_(255)                                            # NaN bit patterns: every partial row that is read was written
    L.call("bags_depth_prior_forward", DEV, C.byref(args), L.ptr(ws), ws.numel(), L.ptr(loss), L.ptr(count), L.ptr(stats))
    g_d = [_place(torch.full((1, H, W), float("nan")), offset) for _ in idx] if want_depth else None
    g_a = [_place(torch.full((1, H, W), float("nan")), offset) for _ in idx] if want_weights else None
    g_t = torch.full((P.N, 2), float("nan"), device=DEV) if (want_table and table is not None) else None
    g_loss = c["cot"].to(DEV)
    L.call("bags_depth_prior_backward", DEV, C.byref(args), L.ptr(stats), L.ptr(g_loss),
           L.ptr_table(g_d) if want_depth else None, L.ptr_table(g_a) if want_weights else None, L.ptr(g_t))
    torch.cuda.synchronize()
    return (loss.cpu(), torch.stack(g_d).cpu() if want_depth else None, torch.stack(g_a).cpu() if want_weights else None,
            None if g_t is None else g_t.cpu(), count.cpu(), stats.cpu())


# ---------------------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("mode,space", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("V", P.VIEWS)
@pytest.mark.parametrize("H,W", P.SHAPES, ids=["%dx%d" % s for s in P.SHAPES])
def test_values_against_float64(H, W, V, mode, space, offset):
    """Loss per view, dL/dD and dL/dA per pixel and the listed table rows within the bars of depth_prior_cases.bars; the test prints
    the margins (largest error over bar; profiles/depth_prior/NOTES.md has their maximum).  Invalid pixels and unlisted rows
    are exact zeros (their bars are 0).  17 views are two launches of each kernel; the aligned run of a shape with W % 4 == 0 is the
    vector path, every other run the scalar path."""
    c = P.make_case(H, W, V, mode, space)
    res = _run(c, offset)
    assert all(torch.isfinite(t).all() for t in res if t is not None)
    ref = P.reference(H, W, V, mode, space)
    assert ((res[4].double() - ref[4]).abs() <= P.EPS32 * ref[4]).all()                  # count = n, rounded once
    valid = P._pieces(c)["valid"][:, None]
    assert res[1][~valid].abs().max().item() == 0.0 and res[2][~valid].abs().max().item() == 0.0 if (~valid).any() else True
    m = P.margins(H, W, V, mode, space, _got(c, res))
    print("\n%dx%d V=%d %s %s %s: margins %s" % (H, W, V, mode, space, "offset" if offset else "aligned",
                                                 "  ".join("%s %.3f" % (n, x) for n, x in zip([n for n in NAMES if n != "dL/dtable" or mode == "l1"], m))))
    assert all(x <= 1.0 for x in m), m                        # (a NaN fails)


# ---------------------------------------------------------------------------------------------------------------- bitwise
def _same(a, b, what=""):
    for x, y, name in zip(a, b, NAMES + ("count",)):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert torch.equal(x, y), (what, name)


@pytest.mark.parametrize("mode,space", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("V", (2, 17))
@pytest.mark.parametrize("H,W", VECTOR_SHAPES, ids=["%dx%d" % s for s in VECTOR_SHAPES])
def test_vector_path_equals_scalar_path(H, W, V, mode, space):
    c = P.make_case(H, W, V, mode, space)
    _same(_run(c, offset=False), _run(c, offset=True))


@pytest.mark.parametrize("mode,space", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("H,W", ((17, 67), P.STRIDED), ids=("17x67", "strided"))
def test_a_view_of_a_16_view_call_equals_its_own_call(H, W, mode, space):
    c = P.make_case(H, W, 16, mode, space)
    loss, gD, gA, gT, count = _run(c)
    for v in (0, 6, 15):
        l1, d1, a1, t1, n1 = _run(c, views=[v])
        assert torch.equal(l1[0], loss[v]) and torch.equal(n1[0], count[v]) and torch.equal(d1[0], gD[v]) and torch.equal(a1[0], gA[v])
        if gT is not None:
            r = c["rows"][v]
            assert torch.equal(t1[r], gT[r]) and t1[[i for i in range(P.N) if i != r]].abs().max().item() == 0.0


@pytest.mark.parametrize("mode,space", (("pearson", "inverse"), ("l1", "depth")))
def test_repeats_bit_for_bit_also_on_a_side_stream(mode, space):
    c = P.make_case(*P.STRIDED, 16, mode, space)
    first, again = _run(c), _run(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _run(c)
    torch.cuda.current_stream().wait_stream(side)
    _same(first, again)
    _same(first, third)


@pytest.mark.parametrize("mode,space", COMBOS, ids=COMBO_IDS)
def test_a_scaled_cotangent_scales_the_gradients_exactly(mode, space):
    c = P.make_case(*P.STRIDED, 2, mode, space)
    full, eighth = _run(c), _run(c, scale=0.125)
    assert torch.equal(eighth[0], full[0]) and torch.equal(eighth[1], full[1] * 0.125) and torch.equal(eighth[2], full[2] * 0.125)
    assert full[3] is None or torch.equal(eighth[3], full[3] * 0.125)


@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("mode,space", (("pearson", "inverse"), ("pearson", "depth"), ("l1", "inverse")))
@pytest.mark.parametrize("H,W", ((17, 67), P.STRIDED), ids=("17x67", "strided"))
def test_each_output_alone_equals_the_full_call(H, W, mode, space, offset):
    """Through the C entries with real NULLs; the buffers are pre-filled with NaN, so every element that must be written was."""
    c = P.make_case(H, W, 16, mode, space)
    full = _c_calls(c, offset, True, True, True)
    assert all(torch.isfinite(t).all() for t in full if t is not None)
    only_d, only_a, only_t = _c_calls(c, offset, True, False, False), _c_calls(c, offset, False, True, False), _c_calls(c, offset, False, False, True)
    assert only_d[2] is None and only_d[3] is None and only_a[1] is None and only_t[1] is None and only_t[2] is None
    assert torch.equal(only_d[1], full[1]) and torch.equal(only_a[2], full[2])
    assert (full[3] is None) == (mode == "pearson") and (full[3] is None or torch.equal(only_t[3], full[3]))
    assert torch.equal(only_t[5], full[5]) and tuple(full[5].shape) == (16, 8) and (full[5][:, 7] == 0).all()
    _same(_run(c, offset), full[:5])                          # and autograd is those calls


# ---------------------------------------------------------------------------------------------------------------- degenerate views
@pytest.mark.parametrize("offset", (False, True), ids=("aligned", "offset"))
@pytest.mark.parametrize("mode,space", COMBOS, ids=COMBO_IDS)
def test_degenerate_views(mode, space, offset):
    """Loss 0, zero gradients and finite values for the views depth_prior_cases.degenerate_case marks; every view within the bars
    of the rule; and the twelve ordinary views bit for bit what a call without the four gives."""
    c = P.degenerate_case(mode, space)
    res = _run(c, offset)
    assert all(torch.isfinite(t).all() for t in res if t is not None)
    got = _got(c, res)
    for v in c["degenerate"]:
        assert res[0][v] == 0 and res[1][v].abs().max() == 0 and res[2][v].abs().max() == 0, v
        assert got[3] is None or got[3][v].abs().max() == 0
    k = P.DEGENERATE_VIEWS
    assert res[4][k["none_valid"]] == 0 and res[4][k["mask_zero"]] == 0 and res[4][k["one_valid"]] == 0.625
    r64, r32 = P.run_torch(c, F64), P.run_torch(c, F32)
    m = P.margins_of(P.bars_of(c, r64, r32), r64, got)
    print("\ndegenerate %s %s: margins %s" % (mode, space, m))
    assert all(x <= 1.0 for x in m), m
    keep = [v for v in range(16) if v not in k.values()]
    without = _run(c, offset, views=keep)
    assert torch.equal(without[0], res[0][keep]) and torch.equal(without[1], res[1][keep]) and torch.equal(without[2], res[2][keep])
    assert torch.equal(without[4], res[4][keep])
    if res[3] is not None:
        rows = [c["rows"][v] for v in keep]
        assert torch.equal(without[3][rows], res[3][rows])


# ---------------------------------------------------------------------------------------------------------------- autograd
def test_no_grad_keeps_nothing_and_constants_give_no_graph():
    c = P.make_case(37, 259, 2, "pearson", "inverse")
    Ds, As, ps, ms = _maps(c, [0, 1], False)
    loss, count = depth_prior_loss(Ds, As, ps, ms)
    assert loss.grad_fn is None and not loss.requires_grad and count.grad_fn is None             # constant inputs
    del loss, count
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    for t in Ds + As:
        t.requires_grad_(True)
    with torch.no_grad():
        loss, count = depth_prior_loss(Ds, As, ps, ms)
    assert loss.grad_fn is None and not loss.requires_grad
    del loss, count
    assert torch.cuda.memory_allocated() == held              # nothing was saved
    loss, count = depth_prior_loss(Ds, As, ps, ms)
    assert loss.grad_fn is not None and type(loss.grad_fn).__name__.startswith("_DepthPrior") and not count.requires_grad
    only_depth = depth_prior_loss(Ds[0], As[0].detach(), ps[0])[0]
    only_depth.sum().backward()
    assert Ds[0].grad is not None and As[0].grad is None
    with pytest.raises(RuntimeError, match="AMD GPU"):
        depth_prior_loss(c["D"][0], As[0], ps[0])             # a host map into the HIP path: refused, not copied
    with pytest.raises(TypeError, match=r"\.float\(\)"):
        depth_prior_loss(Ds[0], As[0], ps[0], ms[0] > 0)


@pytest.mark.parametrize("space", P.SPACES)
def test_bank_on_the_gpu_matches_the_host_copy_and_trains_with_one_adam(space):
    H, W, V = 37, 259, 2
    c = P.make_case(H, W, V, "l1", space)
    host, dev = DepthPriorBank(P.N), DepthPriorBank(P.N, DEV)
    with torch.no_grad():
        host.table.copy_(c["table"])
        dev.table.copy_(c["table"])
    assert dev.table.is_cuda and len(dev) == P.N
    hD, hA = [c["D"][i].clone().requires_grad_(True) for i in range(V)], [c["A"][i].clone().requires_grad_(True) for i in range(V)]
    dD, dA = [c["D"][i].to(DEV).requires_grad_(True) for i in range(V)], [c["A"][i].to(DEV).requires_grad_(True) for i in range(V)]
    lh, nh = host.loss(hD, hA, list(c["prior"]), c["rows"], list(c["mask"]), space=space, min_weight=P.MIN_WEIGHT)
    ld, nd = dev.loss(dD, dA, [t.to(DEV) for t in c["prior"]], c["rows"], [t.to(DEV) for t in c["mask"]], space=space, min_weight=P.MIN_WEIGHT)
    (lh * c["cot"]).sum().backward()
    (ld * c["cot"].to(DEV)).sum().backward()
    bar = P.bars(H, W, V, "l1", space)
    assert ((ld.detach().cpu() - lh.detach()).abs().double() <= bar[0]).all() and torch.equal(nd.cpu(), nh)
    for i in range(V):
        assert ((dD[i].grad.cpu() - hD[i].grad).abs().double() <= bar[1][i]).all()
        assert ((dA[i].grad.cpu() - hA[i].grad).abs().double() <= bar[2][i]).all()
    gd, gh = dev.table.grad.cpu(), host.table.grad
    assert ((gd - gh)[c["rows"]].abs().double() <= bar[3]).all()
    other = [r for r in range(P.N) if r not in c["rows"]]
    assert gd[other].abs().max().item() == 0.0 and (gd[c["rows"]] != 0).all()
    before = dev.table.detach().clone()
    torch.optim.Adam([dev.table], lr=0.01).step()
    moved = (dev.table.detach() != before).cpu()
    assert moved[c["rows"]].all() and not moved[other].any()
    # pearson through the bank does not read the table
    lp = dev.loss(dD[0].detach(), dA[0].detach(), c["prior"][0].to(DEV), c["rows"][0], mode="pearson", space=space)[0]
    assert torch.equal(lp, depth_prior_loss(dD[0].detach(), dA[0].detach(), c["prior"][0].to(DEV), space=space)[0])


# ---------------------------------------------------------------------------------------------------------------- chain
@pytest.mark.parametrize("mode", P.MODES)
def test_chain_with_the_real_operator(mode):
    """rasterize(depth_weights_grad=True) -> depth_prior_loss -> backward reaches means3D, the opacities and the viewmatrix.  Held to
    the same chain with depth_prior_loss_torch in the middle -- in float64 for the reference, in float32 on the GPU for the float32
    path's own error -- by the rule: 4 x that error plus 16 float32 epsilons x (1 + |reference|) per element; the rasterizer is the
    same on all three sides.  min_weight is the threshold tests/test_depth_prior_cpu.py holds to the oracle's weights map."""
    from bags_raster import GaussianRasterizer
    from scenes import camera_tensors, hip_settings, make_case
    scene, cam = make_case(24, 32, 32, 3.0, 1, seed=5, dist=3.0)
    H, W = cam.image_height, cam.image_width
    table = torch.tensor([[1.0, 0.0], [0.9, 0.02], [1.1, -0.01]], device=DEV)

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
    g = torch.Generator().manual_seed(31)
    prior = (weights0[0] / depth0[0]).cpu() * (1.0 + 0.1 * torch.randn(H, W, generator=g).clamp(-3, 3))
    prior[torch.rand(H, W, generator=g) < 0.05] = 0.0
    mask = torch.where(torch.rand(H, W, generator=g) < 0.1, 0.0, 1.0) * (0.25 + 0.75 * torch.rand(H, W, generator=g))
    prior, mask = prior.to(DEV), mask.to(DEV)
    valid = (mask > 0) & (weights0[0] >= P.CHAIN_MIN_WEIGHT) & (depth0[0] > 0) & (prior > 0)
    assert valid.float().mean().item() >= 0.25 and (weights0[0] - P.CHAIN_MIN_WEIGHT).abs().min().item() >= 5e-4

    def chain(middle):
        t, ct, depth, weights = render()
        assert depth.requires_grad and weights.requires_grad
        kw = dict(mode=mode, space="inverse", min_weight=P.CHAIN_MIN_WEIGHT)
        if mode == "l1":
            kw.update(table=table, rows=[1])
        loss, count = middle(depth, weights, kw)
        loss.sum().backward()
        torch.cuda.synchronize()
        return dict(loss=loss.detach().double().cpu(), count=count.double().cpu(), means3D=t["means3D"].grad.cpu(),
                    opacities=t["opacities"].grad.cpu(), viewmatrix=ct["viewmatrix"].grad.cpu())

    hip = chain(lambda d, a, kw: depth_prior_loss(d, a, prior, mask, **kw))
    t32 = chain(lambda d, a, kw: depth_prior_loss_torch(d, a, prior, mask, **kw))
    t64 = chain(lambda d, a, kw: depth_prior_loss_torch(d.double(), a.double(), prior.double(), mask.double(),
                                                        **{**kw, **({"table": table.double()} if mode == "l1" else {})}))
    assert t64["count"].item() > 0 and all(abs(r["count"].item() - t64["count"].item()) <= P.EPS32 * t64["count"].item() for r in (hip, t32))
    worst = {}
    for name in ("loss", "means3D", "opacities", "viewmatrix"):
        got, r32, r64 = hip[name].double(), t32[name].double(), t64[name].double()
        assert torch.isfinite(got).all() and got.abs().max().item() > 0 and r64.abs().max().item() > 0, name
        bar = P.FACTOR * (r32 - r64).abs() + P.FLOOR_EPS * P.EPS32 * (1 + r64.abs())
        worst[name] = float(((got - r64).abs() / bar).max())
    print("\nchain %s margins:" % mode, {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst       # (a NaN fails)
