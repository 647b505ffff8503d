"""GPU checks of bags_raster.depth_smooth_loss / normal_smooth_loss (csrc/smooth.hip) against their PyTorch statements in float64 on
the case images of tests/smooth_cases.py: every size for 1, 5 and 17 views over both front-ends, both orders, both penalties,
normalize on / off, both spaces, with and without guide and mask; holes, an empty view and a plane; bit-for-bit repeats, independence
of the neighbours, of the storage offset and of the outputs wanted; and the version check of the saved maps."""
import functools

import pytest
import torch

import smooth_cases as M
from bags_raster import depth_smooth_loss, depth_smooth_loss_torch, normal_smooth_loss, normal_smooth_loss_torch
from scenes import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
HIP = {False: depth_smooth_loss, True: normal_smooth_loss}
TORCH = {False: depth_smooth_loss_torch, True: normal_smooth_loss_torch}


@functools.lru_cache(maxsize=None)
def _reference(name, H, W, V, key, normals):
    """The float64 statement on the CPU, computed once per case and configuration: shared by the tests, never written to."""
    return M.forward_backward(TORCH[normals], name, H, W, V, dict(key), normals, F64, "cpu")


def _hip(name, H, W, V, cfg, normals):
    loss, count, gF, gA = M.forward_backward(HIP[normals], name, H, W, V, cfg, normals, F32, DEV)
    torch.cuda.synchronize()
    return loss.cpu(), count.cpu(), [g.cpu() for g in gF], [g.cpu() for g in gA]


def _check(name, H, W, V, cfg, normals, gradient_bar=True):
    """Loss and count <= 1e-5 (1 + |x|) against the float64 statement, the gradients of every view <= 1e-4 (scenes.rel_err) against
    float64 autograd, exact zeros where the reference has exact zeros.  Returns the worst error over bar, and the results."""
    l64, n64, f64, a64 = _reference(name, H, W, V, M.key_of(cfg), normals)
    loss, count, gF, gA = _hip(name, H, W, V, cfg, normals)
    assert loss.shape == (V,) and count.shape == (V,) and loss.dtype == F32 and torch.isfinite(loss).all()
    e_l = ((loss.double() - l64).abs() / (1 + l64.abs())).max().item()
    e_n = ((count.double() - n64).abs() / (1 + n64.abs())).max().item()
    e_g = 0.0
    for v in range(V):
        for got, ref in ((gF[v], f64[v]), (gA[v], a64[v])):
            assert got.shape == ref.shape and torch.isfinite(got).all()
            if gradient_bar:
                assert (got[ref == 0] == 0).all()                       # pixels that are not usable: exact zeros
                e_g = max(e_g, rel_err(got, ref))
    tag = " ".join("%s=%s" % kv for kv in sorted(cfg.items()))
    print("\n%s %s %dx%d V=%d %s: loss %.2e  count %.2e  gradient %.2e" % ("normal" if normals else "depth", name, H, W, V, tag, e_l, e_n, e_g))
    assert e_l <= 1e-5 and e_n <= 1e-5 and e_g <= 1e-4
    return max(e_l / 1e-5, e_n / 1e-5, e_g / 1e-4), (loss, count, gF, gA)


@pytest.mark.parametrize("V", M.VIEWS)
@pytest.mark.parametrize("H,W", M.SIZES)
def test_every_size_over_the_combinations(H, W, V):
    eps = M.eps_l1_of(H, W, V)
    worst = max([_check("generic", H, W, V, cfg, False)[0] for cfg in M.depth_configs(eps)]
                + [_check("generic", H, W, V, cfg, True)[0] for cfg in M.normal_configs(eps)])
    print("generic %dx%d V=%d: worst error over bar %.3f" % (H, W, V, worst))


@pytest.mark.parametrize("normals", (False, True))
def test_holes_get_exact_zeros(normals):
    for (H, W, V) in M.HOLES_SIZES:
        kind = M.hole_kind(H, W)
        dead = torch.zeros(H, W, dtype=torch.bool)
        for k in M.unusable_kinds(normals):
            dead |= kind == k
        for cfg in (M.HOLES_CONFIGS[:2] if normals else M.HOLES_CONFIGS):
            _, (loss, count, gF, gA) = _check("holes", H, W, V, cfg, normals)
            assert (count > 0).all()
            for v in range(V):
                assert (gF[v][:, dead] == 0).all() and (gA[v][:, dead] == 0).all() and gF[v][:, kind > 4].abs().max() > 0


@pytest.mark.parametrize("H,W", ((1, 1), (5, 7), (64, 256)))
def test_an_empty_view_and_one_pixel_are_zero_not_nan(H, W):
    for normals in (False, True):
        for cfg in (M.config(order=1), M.config(order=2, penalty="l2", normalize=not normals, guide="none", masked=False)):
            names = ("empty", "generic") if (H, W) == (1, 1) else ("empty",)
            for name in names:
                _, (loss, count, gF, gA) = _check(name, H, W, 5, cfg, normals)
                assert (loss == 0).all() and (count == 0).all() and all((g == 0).all() for g in gF + gA)


@pytest.mark.parametrize("H,W", ((5, 7), (33, 70), (64, 256)))
def test_the_second_order_is_zero_on_a_plane(H, W):
    """d is the float32 error of x there (in the float64 reference too, whose inputs are the float32 maps), so the gradients are
    held to be finite, not to the reference's."""
    for normalize in (True, False):
        _, (loss, count, gF, gA) = _check("plane", H, W, 5, M.config(order=2, eps=1e-3, normalize=normalize), False, gradient_bar=False)
        assert (count > 0).all() and (loss.abs() <= 1e-8).all()


def _run(fn, Fs, As, Gs, ms, kw, wanted=None):
    """(loss, count, gradients of the wanted inputs) on the GPU."""
    loss, count = fn(Fs, As, Gs, ms, **kw)
    wanted = [t for t in Fs + As if t.requires_grad] if wanted is None else wanted
    gs = torch.autograd.grad(loss, wanted, M.cotangent(len(Fs)).to(DEV, F32), allow_unused=True)
    return (loss.detach(), count) + tuple(gs)


def _same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("normals", (False, True))
def test_two_runs_give_the_same_bits(normals):
    for cfg in (M.config(order=1), M.config(order=2, eps=1e-3, guide="gray")):
        a, b = _hip("holes", 33, 70, 17, cfg, normals), _hip("holes", 33, 70, 17, cfg, normals)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and _same(a[2], b[2]) and _same(a[3], b[3])


@pytest.mark.parametrize("normals", (False, True))
def test_a_view_does_not_depend_on_its_neighbours(normals):
    """View 3 alone, in a 5-view call, as [3, 7] and as the last of 17 (the second chunk): the same loss, count and gradients, bit
    for bit."""
    for (H, W) in ((64, 256), (33, 70)):
        for cfg in (M.config(order=1), M.config(order=2, penalty="l2", guide="gray")):
            results = []
            for order in ([3], [0, 1, 2, 3, 4], [3, 7], list(range(4, 17)) + [0, 1, 2, 3]):
                Fs, As, Gs, ms, kw = M.arguments("generic", H, W, 17, cfg, normals, F32, DEV, views=order)
                loss, count = HIP[normals](Fs, As, Gs, ms, **kw)
                at = order.index(3)
                gs = torch.autograd.grad(loss[at], [Fs[at], As[at]], allow_unused=True)
                assert (gs[1] is None) == normals
                results.append((loss[at].detach(), count[at]) + gs)
            for r in results[1:]:
                assert _same(r, results[0])


@pytest.mark.parametrize("normals", (False, True))
def test_a_storage_offset_of_one_element_gives_the_same_bits(normals):
    """Maps that are not 16-byte aligned: the kernels load element by element."""
    H, W = 64, 256
    for cfg in (M.config(order=1), M.config(order=2, guide="gray")):
        def run(shift):
            def place(t):
                buf = torch.empty(t.numel() + 4, device=DEV)
                v = buf[shift:shift + t.numel()].view(t.shape)
                v.copy_(t.detach())
                return v
            Fs, As, Gs, ms, kw = M.arguments("generic", H, W, 2, cfg, normals, F32, DEV)
            Fs, As = [place(t).requires_grad_() for t in Fs], [place(t).requires_grad_() for t in As]
            Gs, ms = [place(t) for t in Gs], [place(t) for t in ms]
            assert all(t.data_ptr() % 16 == 4 * shift for t in Fs + As + Gs + ms)
            return _run(HIP[normals], Fs, As, Gs, ms, kw)
        assert _same(run(0), run(1))


def test_what_is_stored_does_not_depend_on_what_is_wanted():
    for cfg in (M.config(order=1), M.config(order=2, space="depth", normalize=False, penalty="l2")):
        Fs, As, Gs, ms, kw = M.arguments("holes", 33, 70, 5, cfg, False, F32, DEV)
        both = _run(depth_smooth_loss, Fs, As, Gs, ms, kw)
        only_d = _run(depth_smooth_loss, Fs, [t.detach() for t in As], Gs, ms, kw, wanted=Fs)
        only_a = _run(depth_smooth_loss, [t.detach() for t in Fs], As, Gs, ms, kw, wanted=As)
        assert _same(both[:2], only_d[:2]) and _same(both[:2], only_a[:2])
        assert _same(both[2:7], only_d[2:]) and _same(both[7:], only_a[2:])
        # one view's depth alone
        part = _run(depth_smooth_loss, [Fs[0].detach(), Fs[1]] + [t.detach() for t in Fs[2:]], [t.detach() for t in As], Gs, ms, kw, wanted=[Fs[1]])
        assert torch.equal(part[2], both[3])


@pytest.mark.parametrize("normals", (False, True))
def test_an_in_place_write_to_a_saved_map_raises(normals):
    for victim in range(4):
        Fs, As, Gs, ms, kw = M.arguments("generic", 5, 7, 1, M.config(), normals, F32, DEV)
        maps = [Fs[0] * 1.0, As[0] * 1.0, Gs[0].clone(), ms[0].clone()]
        loss, _ = HIP[normals](maps[0], maps[1], maps[2], maps[3], **kw)
        with torch.no_grad():
            maps[victim].mul_(1.0)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            loss.sum().backward()


def test_no_gradient_wanted_keeps_nothing_and_count_is_constant():
    Fs, As, Gs, ms, kw = M.arguments("generic", 33, 70, 5, M.config(), False, F32, DEV)
    with torch.no_grad():
        loss, count = depth_smooth_loss(Fs, As, Gs, ms, **kw)
    assert not loss.requires_grad and not count.requires_grad
    loss2, count2 = depth_smooth_loss(Fs, As, Gs, ms, **kw)
    assert loss2.requires_grad and not count2.requires_grad and torch.equal(loss, loss2.detach()) and torch.equal(count, count2)
