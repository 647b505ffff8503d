"""GPU checks of bags_raster.alpha_loss (csrc/alpha.hip) against its PyTorch statement in float64 on the CPU, on the case images of
tests/alpha_cases.py: every size in all four modes, with and without a mask, for 1, 5 and 17 views; holes, views without a usable
pixel and the pixels placed at the clamp; bit-for-bit repeats, independence of the neighbours, the vector against the element
instance, stale scratch, the memory contract (tests/fenced.py), the version check of the saved maps, and the term driving the
Gaussians through the operator.

Bars, those of the sibling losses (tests/test_normal_map_gpu.py): loss and count <= 1e-5 (1 + |x|), every view's gradient <= 1e-4 by
scenes.rel_err, exact zeros wherever the reference has exact zeros.  Every check prints its worst error over bar."""
import functools

import pytest
import torch

import alpha_cases as M
from bags_raster import _lib as L
from bags_raster import alpha_loss, alpha_loss_torch
from fenced import fenced
from scenes import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64


@functools.lru_cache(maxsize=None)
def _reference(name, H, W, V, mode, masked):
    """The float64 statement on the CPU, computed once per case: shared by the tests, never written to."""
    return M.forward_backward(alpha_loss_torch, name, H, W, V, mode, masked, F64, "cpu")


def _hip(name, H, W, V, mode, masked):
    loss, count, grads = M.forward_backward(alpha_loss, name, H, W, V, mode, masked, F32, DEV)
    torch.cuda.synchronize()
    return loss.cpu(), count.cpu(), [g.cpu() for g in grads]


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and len(a[2]) == len(b[2]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def _check(name, H, W, V, mode, masked, got=None):
    """``got`` (default: a run of the HIP path) against the float64 statement.  Returns the worst error over bar and the result."""
    l64, n64, g64 = _reference(name, H, W, V, mode, masked)
    loss, count, grads = _hip(name, H, W, V, mode, masked) if got is None else got
    assert loss.shape == (V,) and count.shape == (V,) and loss.dtype == F32 and torch.isfinite(loss).all() and torch.isfinite(count).all()
    e_l = ((loss.double() - l64).abs() / (1 + l64.abs())).max().item()
    e_n = ((count.double() - n64).abs() / (1 + n64.abs())).max().item()
    e_g = 0.0
    for v in range(V):
        assert grads[v].shape == (1, H, W) and torch.isfinite(grads[v]).all()
        assert (grads[v][g64[v] == 0] == 0).all()                       # exact zeros wherever the reference has them
        e_g = max(e_g, rel_err(grads[v], g64[v]))
    over = max(e_l / 1e-5, e_n / 1e-5, e_g / 1e-4)
    print("\n%s %dx%d V=%d %s %s: loss %.2e  count %.2e  gradient %.2e  worst error over bar %.3f" %
          (name, H, W, V, mode, "mask" if masked else "no mask", e_l, e_n, e_g, over))
    assert e_l <= 1e-5 and e_n <= 1e-5 and e_g <= 1e-4
    return over, (loss, count, grads)


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("V", M.VIEWS)
@pytest.mark.parametrize("H,W", M.SIZES)
def test_every_size_in_every_mode_with_and_without_a_mask(H, W, V):
    worst = max(_check("generic", H, W, V, mode, masked)[0] for mode in M.MODES for masked in (False, True))
    print("generic %dx%d V=%d: worst error over bar %.3f" % (H, W, V, worst))


@pytest.mark.parametrize("mode", M.MODES)
def test_holes_get_exact_zeros_and_the_others_do_not(mode):
    H, W = 33, 70
    kind = M.hole_kind(H, W)
    for masked in (True, False):
        bad = torch.isin(kind, torch.tensor(M.unusable_kinds(mode, masked)))
        _, (loss, count, grads) = _check("holes", H, W, 5, mode, masked)
        assert (count > 0).all()
        for v in range(5):
            assert (grads[v][0][bad] == 0).all() and (grads[v][0][~bad] != 0).all()
    _check("holes", 5, 7, 17, mode, True)
    _check("holes", 1, 1, 1, mode, True)                                 # the only pixel is a NaN: an empty view


@pytest.mark.parametrize("H,W", ((1, 1), (5, 7), (64, 256)))
def test_a_view_without_a_usable_pixel_is_zero_not_nan(H, W):
    for mode in M.MODES:
        for masked in (False, True):
            _, (loss, count, grads) = _check("empty", H, W, 5, mode, masked)
            assert (loss[0::2] == 0).all() and (count[0::2] == 0).all() and all((g == 0).all() for g in grads[0::2])
            assert (count[1::2] > 0).all() and all(torch.isfinite(g).all() for g in grads)


@pytest.mark.parametrize("H,W", ((3, 3), (5, 7), (33, 70)))
def test_the_pixels_placed_at_the_clamp_decide_as_the_reference(H, W):
    for mode in M.MODES:
        _, (loss, count, grads) = _check("edges", H, W, 5, mode, True)
        g64 = _reference("edges", H, W, 5, mode, True)[2]
        for v in range(5):
            # (the seventh pixel, A == t, is l1's and l2's: in bce the rule's (a - t) / (a (1 - a)) is an exact 0 there, while autograd
            # adds two terms that cancel to an ulp)
            n = 6 if mode in M.CLAMPED else 7
            got, want = grads[v].reshape(-1)[:n], g64[v].reshape(-1)[:n]
            assert torch.equal(got != 0, want != 0), (mode, v, got, want)
            if mode in M.CLAMPED:
                assert torch.equal((got != 0)[:6], torch.tensor(M.EDGES["inside"][:6]))


def test_the_default_eps_against_the_statement_on_the_same_maps():
    """eps = 1e-4 is no float32 number: the statement rounds lo and hi to the dtype of the maps, so the float64 run of the cases clamps
    at another a than a float32 run (alpha_cases).  Here the default eps, held to the statement on the float32 maps themselves (whose
    arithmetic after the loads is float64 too), under the same bars."""
    H, W, V = 33, 70, 5
    c = M.case("generic", H, W, V)
    for mode in M.CLAMPED:
        out = []
        for fn, dev in ((alpha_loss_torch, "cpu"), (alpha_loss, DEV)):
            As = [x.to(dev).requires_grad_() for x in c["weights"]]
            loss, count = fn(As, None if mode == "entropy" else [x.to(dev) for x in c["target"]], [x.to(dev) for x in c["mask"]], mode=mode)
            gs = torch.autograd.grad(loss, As, M.cotangent(V).float().to(dev))
            out.append((loss.detach().cpu().double(), count.cpu().double(), [g.cpu() for g in gs]))
        (l_t, n_t, g_t), (l_h, n_h, g_h) = out
        e_l, e_n = ((l_h - l_t).abs() / (1 + l_t.abs())).max().item(), ((n_h - n_t).abs() / (1 + n_t.abs())).max().item()
        e_g = max(rel_err(a, b) for a, b in zip(g_h, g_t))
        print("\ndefault eps %s: loss %.2e  count %.2e  gradient %.2e" % (mode, e_l, e_n, e_g))
        assert e_l <= 1e-5 and e_n <= 1e-5 and e_g <= 1e-4 and all(torch.equal(a == 0, b == 0) for a, b in zip(g_h, g_t))


# ------------------------------------------------------------------------------------------------------------------ bits
def test_two_runs_give_the_same_bits():
    for mode in M.MODES:
        assert _same(_hip("holes", 33, 70, 17, mode, True), _hip("holes", 33, 70, 17, mode, True))
        assert _same(_hip("generic", 17, 67, 5, mode, False), _hip("generic", 17, 67, 5, mode, False))


def test_a_view_does_not_depend_on_its_neighbours():
    """View 3 in a 17-view call, alone, and as the only member of the call's second batch of 16: the same loss, count and gradient,
    bit for bit; the float4 instance and, at 33 x 70, its element-wise tail."""
    for (H, W) in ((64, 256), (33, 70), (5, 7)):
        c = M.case("generic", H, W, 17)
        dev = {n: [t.to(DEV) for t in c[n]] for n in ("weights", "target", "mask")}
        for mode in ("bce", "l1"):
            results = []
            for order in (list(range(17)), [3], [v for v in range(17) if v != 3] + [3], [0, 1, 2, 3, 4]):
                As = [dev["weights"][v].clone().requires_grad_() for v in order]
                loss, count = alpha_loss(As, [dev["target"][v] for v in order], [dev["mask"][v] for v in order], mode=mode)
                at = order.index(3)
                (g,) = torch.autograd.grad(loss[at], As[at])
                results.append((loss[at].detach(), count[at], g))
            for r in results[1:]:
                assert all(torch.equal(x, y) for x, y in zip(r, results[0]))


def test_the_vector_and_the_element_instance_give_the_same_bits():
    """Maps 4 bytes into their storage are contiguous but not 16-byte aligned: the call takes the element-by-element kernels."""
    for (H, W) in ((17, 67), (64, 256)):
        c = M.case("generic", H, W, 5)
        for mode in M.MODES:
            def run(shift):
                def place(t):
                    buf = torch.empty(t.numel() + 4, device=DEV)
                    v = buf[shift:shift + t.numel()].view(t.shape)
                    v.copy_(t)
                    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * shift
                    return v
                As = [place(t).requires_grad_() for t in c["weights"][:2]]
                ts = None if mode == "entropy" else [place(t) for t in c["target"][:2]]
                loss, count = alpha_loss(As, ts, [place(t) for t in c["mask"][:2]], mode=mode)
                gs = torch.autograd.grad(loss.sum(), As)
                return loss.detach(), count, [g.clone() for g in gs]
            assert _same(run(0), run(1)), (H, W, mode)


def test_stale_scratch_does_not_reach_a_small_call():
    """A 1 x 1 x 1 call leaves all but one span empty: after a full-size call the scratch it is handed holds that call's rows."""
    for mode in M.MODES:
        _hip("generic", 64, 256, 16, mode, True)
        _check("generic", 1, 1, 1, mode, True)
        _check("generic", 3, 3, 5, mode, False)


# ------------------------------------------------------------------------------------------------------------------ memory
MEMORY_CALLS = (("generic", 33, 70, 17, "bce", True), ("holes", 33, 70, 17, "entropy", False), ("generic", 5, 7, 1, "l1", True))


@pytest.mark.parametrize("dirt", (0xA5, 0xFF))
def test_nothing_outside_its_buffers_and_nothing_of_what_they_held(dirt):
    plain = [_hip(*call) for call in MEMORY_CALLS]
    with fenced(dirt) as f:
        dirty = [_hip(*call) for call in MEMORY_CALLS]
    assert f.intact(), f.report()
    assert f.skipped == 0, f.skipped_what
    assert f.from_package >= 1 and f.workspaces == len(MEMORY_CALLS) and set(f.workspace_bytes) == {L.ALPHA_WORKSPACE_BYTES}
    for a, b, call in zip(plain, dirty, MEMORY_CALLS):
        assert _same(a, b), call
        _check(*call, got=b)


def test_the_workspace_is_taken_as_given():
    call = MEMORY_CALLS[0]
    plain = _hip(*call)
    with fenced(0xA5, shift=16) as f:
        assert _same(_hip(*call), plain)
    assert f.intact(), f.report()
    with fenced(0xA5, shift=4) as f:
        with pytest.raises(RuntimeError, match="not 16-byte aligned"):
            _hip(*call)
    assert f.intact(), f.report()
    with fenced(0xA5, shrink=1) as f:
        with pytest.raises(RuntimeError, match="needs a workspace of %d bytes" % L.ALPHA_WORKSPACE_BYTES):
            _hip(*call)
    assert f.intact(), f.report()


# ------------------------------------------------------------------------------------------------------------------ autograd
def test_an_in_place_write_to_a_saved_map_raises_and_no_grad_saves_nothing():
    c = M.case("generic", 5, 7, 1)
    for victim in ("weights", "target", "mask"):
        t = {n: c[n][0].to(DEV).clone() for n in ("weights", "target", "mask")}
        A = t["weights"].requires_grad_()
        args = dict(weights=A * 1.0, target=t["target"], mask=t["mask"])
        loss, _ = alpha_loss(args["weights"], args["target"], args["mask"])
        with torch.no_grad():
            args[victim].mul_(1.0)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            loss.sum().backward()
    A = c["weights"][0].to(DEV).requires_grad_()
    with torch.no_grad():
        loss, count = alpha_loss(A, mode="entropy")
    assert loss.grad_fn is None and not loss.requires_grad
    loss, count = alpha_loss(A.detach(), c["target"][0].to(DEV))
    assert loss.grad_fn is None
    with pytest.raises(TypeError, match="float32"):
        alpha_loss(A.double(), c["target"][0].to(DEV).double())
    with pytest.raises(RuntimeError, match="contiguous"):
        alpha_loss(torch.zeros(7, 5, device=DEV).t(), c["target"][0].to(DEV))


def test_the_term_drives_the_gaussians_through_the_operator():
    """render_views(depth_weights_grad=True) of two PoseBank cameras at 48 x 64 -> alpha_loss(mode="bce") against a disc silhouette ->
    backward.  The leaf gradients equal those of the same graph with alpha_loss_torch (float32, same device) downstream of the
    operator, within 1e-4 (scenes.rel_err), and are not zero."""
    from bags_raster import GaussianBag, PipelineParams, PoseBank, render_views
    from bags_raster.synth import sphere_views, synth_scene
    H, W = 48, 64
    y, x = torch.meshgrid(torch.arange(H, dtype=F32), torch.arange(W, dtype=F32), indexing="ij")
    disc = (((y - H / 2 + 0.5) ** 2 + (x - W / 2 + 0.5) ** 2) < (0.35 * H) ** 2).float().to(DEV)
    cot = torch.tensor((1.0, 0.5), device=DEV)

    def leaves(fn):
        bag = GaussianBag.from_activated(synth_scene(300, 7, 2.0, 1), 1, device=DEV)
        bank = PoseBank.from_cameras(sphere_views(2, W, H, noise=0.05), device=DEV)
        pkgs = render_views([bank.camera(i) for i in range(2)], bag, PipelineParams(), torch.zeros(3, device=DEV), 0.0, None,
                            depth_weights_grad=True)
        weights = [p["weights"] for p in pkgs]
        assert all(w.requires_grad and w.shape == (1, H, W) for w in weights)
        loss, count = fn(weights, [disc, disc], mode="bce")
        assert (loss > 0).all() and (count == H * W).all()
        (loss * cot).sum().backward()
        torch.cuda.synchronize()
        return [w.detach().cpu() for w in weights], {n: getattr(bag, n).grad.cpu() for n in ("_xyz", "_opacity", "_scaling")}

    maps_hip, g_hip = leaves(alpha_loss)
    maps_torch, g_torch = leaves(alpha_loss_torch)
    assert all(torch.equal(a, b) for a, b in zip(maps_hip, maps_torch))            # the premise: the same operator on both sides
    partly = sum(((a > 0.05) & (a < 0.95)).float().mean().item() for a in maps_hip) / 2
    print("\nchain: %.3f of the pixels partly covered" % partly)
    for n in g_hip:
        e = rel_err(g_hip[n], g_torch[n])
        print("chain: %s gradient %.2e (over bar %.3f), max |g| %.3e" % (n, e, e / 1e-4, g_hip[n].abs().max().item()))
        assert torch.isfinite(g_hip[n]).all() and g_hip[n].abs().max().item() > 0 and e <= 1e-4, n
