"""GPU checks of bags_raster.normal_map_loss (csrc/normal_map.hip) against its PyTorch statement in float64 on the case images of
tests/normal_map_cases.py: every size in both modes, with and without a mask, for 1, 5 and 17 views; holes, an empty view and
depth_to_normal's output as the target; bit-for-bit repeats, independence of the neighbours, and the version check of the saved
maps."""
import functools

import pytest
import torch

import normal_map_cases as M
from bags_raster import depth_to_normal, normal_map_loss, normal_map_loss_torch
from scenes import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64


@functools.lru_cache(maxsize=None)
def _reference(name, H, W, V, mode, masked):
    """The float64 statement on the CPU, computed once per case: shared by the tests, never written to."""
    return M.forward_backward(normal_map_loss_torch, name, H, W, V, mode, masked, F64, "cpu")


def _hip(name, H, W, V, mode, masked):
    loss, count, grads = M.forward_backward(normal_map_loss, name, H, W, V, mode, masked, F32, DEV)
    torch.cuda.synchronize()
    return loss.cpu(), count.cpu(), [g.cpu() for g in grads]


def _check(name, H, W, V, mode, masked):
    """Loss and count <= 1e-5 (1 + |x|) against the float64 statement, the gradient of every view <= 1e-4 (scenes.rel_err) against
    float64 autograd, exact zeros where the reference has exact zeros.  Returns the worst error over bar."""
    l64, n64, g64 = _reference(name, H, W, V, mode, masked)
    loss, count, grads = _hip(name, H, W, V, mode, masked)
    assert loss.shape == (V,) and count.shape == (V,) and loss.dtype == F32 and torch.isfinite(loss).all()
    e_l = ((loss.double() - l64).abs() / (1 + l64.abs())).max().item()
    e_n = ((count.double() - n64).abs() / (1 + n64.abs())).max().item()
    e_g = 0.0
    for v in range(V):
        assert grads[v].shape == (3, H, W) and torch.isfinite(grads[v]).all()
        assert (grads[v][g64[v] == 0] == 0).all()                       # invalid pixels: exact zeros
        e_g = max(e_g, rel_err(grads[v], g64[v]))
    print("\n%s %dx%d V=%d %s %s: loss %.2e  count %.2e  gradient %.2e" % (name, H, W, V, mode, "mask" if masked else "no mask", e_l, e_n, e_g))
    assert e_l <= 1e-5 and e_n <= 1e-5 and e_g <= 1e-4
    return max(e_l / 1e-5, e_n / 1e-5, e_g / 1e-4), (loss, count, grads)


@pytest.mark.parametrize("V", M.VIEWS)
@pytest.mark.parametrize("H,W", M.SIZES)
def test_every_size_in_both_modes_with_and_without_a_mask(H, W, V):
    worst = max(_check("generic", H, W, V, mode, masked)[0] for mode in ("cos", "l1") for masked in (False, True))
    print("generic %dx%d V=%d: worst error over bar %.3f" % (H, W, V, worst))


@pytest.mark.parametrize("mode", ("cos", "l1"))
def test_holes_get_exact_zeros(mode):
    H, W = 33, 70
    kind = M.hole_kind(H, W)
    _, (loss, count, grads) = _check("holes", H, W, 5, mode, True)
    assert (count > 0).all()
    for v in range(5):
        assert (grads[v][:, kind <= 4] == 0).all() and grads[v][:, kind > 4].abs().max() > 0
    _check("holes", 5, 7, 17, mode, False)


@pytest.mark.parametrize("H,W", ((1, 1), (5, 7), (64, 256)))
def test_an_empty_view_is_zero_not_nan(H, W):
    for mode in ("cos", "l1"):
        _, (loss, count, grads) = _check("empty", H, W, 5, mode, True)
        assert (loss == 0).all() and (count == 0).all() and all((g == 0).all() for g in grads)


@pytest.mark.parametrize("H,W", ((3, 3), (33, 70), (64, 256)))
def test_depth_to_normal_as_the_target(H, W):
    for mode in ("cos", "l1"):
        _, (loss, count, grads) = _check("depth_target", H, W, 5, mode, False)
        assert (count > 0).all() and (count <= (H - 2) * (W - 2)).all()      # the border has no depth normal: "no target here"
    # and straight from the kernel that makes the target: the zeros at its invalid pixels fall under the prior rule
    c = M.case("depth_target", H, W, 5)
    A = c["weights"][0].to(DEV)
    z = 2.0 + 0.3 * torch.arange(W, device=DEV)[None, :] / W + 0.2 * torch.arange(H, device=DEV)[:, None] / H
    target, valid = depth_to_normal(A * z[None], A, (float(W), float(W), W / 2 - 0.5, H / 2 - 0.5))
    N = c["normal"][0].to(DEV).requires_grad_()
    loss, count = normal_map_loss(N, A, target)
    loss.backward()
    assert count.item() == valid.sum().item() and (N.grad[:, ~valid] == 0).all() and torch.isfinite(N.grad).all()


def test_two_runs_give_the_same_bits():
    for mode in ("cos", "l1"):
        a, b = _hip("holes", 33, 70, 17, mode, True), _hip("holes", 33, 70, 17, mode, True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_a_view_does_not_depend_on_its_neighbours():
    """View 3 alone, in a 5-view call and as the 17th view's chunk-mate: the same loss, count and gradient, bit for bit; both the
    float4 instance (W % 4 == 0) and the element-by-element one."""
    for (H, W) in ((64, 256), (33, 70)):
        c = M.case("generic", H, W, 17)
        dev = {n: [t.to(DEV) for t in ts] for n, ts in c.items()}
        results = []
        for order in ([3], [0, 1, 2, 3, 4], [3, 7], list(range(4, 17)) + [0, 1, 2, 3]):
            Ns = [dev["normal"][v].clone().requires_grad_() for v in order]
            loss, count = normal_map_loss(Ns, [dev["weights"][v] for v in order], [dev["target"][v] for v in order],
                                          [dev["mask"][v] for v in order], mode="l1")
            at = order.index(3)
            (g,) = torch.autograd.grad(loss[at], Ns[at])
            results.append((loss[at].detach(), count[at], g))
        for r in results[1:]:
            assert all(torch.equal(x, y) for x, y in zip(r, results[0]))


def test_the_vector_and_the_element_instance_give_the_same_bits():
    """An unaligned view of the same data takes the element-by-element kernels."""
    H, W = 64, 256
    c = M.case("generic", H, W, 1)
    N, A, p, m = (c[n][0].to(DEV) for n in ("normal", "weights", "target", "mask"))

    def run(shift):
        def place(t):
            buf = torch.empty(t.numel() + 4, device=DEV)
            v = buf[shift:shift + t.numel()].view(t.shape)
            v.copy_(t)
            return v
        Nl = place(N).requires_grad_()
        loss, count = normal_map_loss(Nl, place(A), place(p), place(m))
        (g,) = torch.autograd.grad(loss, Nl)
        return loss.detach(), count, g
    a, b = run(0), run(1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_an_in_place_write_to_a_saved_map_raises():
    c = M.case("generic", 5, 7, 1)
    for victim in ("normal", "weights", "target", "mask"):
        t = {n: c[n][0].to(DEV).clone() for n in c}
        N = t["normal"].requires_grad_()
        Nin = N * 1.0
        args = dict(normal=Nin, weights=t["weights"], target=t["target"], mask=t["mask"])
        loss, _ = normal_map_loss(args["normal"], args["weights"], args["target"], args["mask"])
        with torch.no_grad():
            args[victim].mul_(1.0)
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            loss.sum().backward()
