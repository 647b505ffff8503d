"""tests/camera_cases.py before it judges a kernel: the case generator gives what its names say, the float64 chain has the
properties of a camera, its gradients are the central differences of its values, and the float32 chain that sets the bar is a usable
yardstick on every case."""
import math

import pytest
import torch

import camera_cases as CC
from bags_raster import camera as cam

NO_ALIGNMENT = [n for n in CC.CASES if CC.make_case(n)[0]["grot"] is None and CC.make_case(n)[0]["gscale"] is None]


def test_cases_are_what_their_names_say():
    f32 = lambda t: torch.equal(t.to(torch.float32).to(torch.float64), t)
    for name in CC.CASES:
        inp, cots = CC.make_case(name)
        assert [tuple(c.shape) for c in cots] == [(4, 4), (4, 4), (4, 4), (3,)]
        for t in list(inp.values()) + cots:                  # float64 tensors holding float32 numbers
            if torch.is_tensor(t):
                assert t.dtype == torch.float64 and f32(t) and torch.isfinite(t).all(), name
        again, cots_again = CC.make_case(name)               # seeded
        assert all(torch.equal(a, b) for a, b in zip(cots, cots_again)) and torch.equal(inp["dq"], again["dq"])
        worst = max(CC.scalar_cancellation(inp, cots).values())  # the scalar gradients' sums do not cancel (benign: g_fovy, 18-fold)
        assert worst <= CC.MAX_CANCELLATION or (name == "benign" and worst < 20), (name, worst)
    q = lambda n: CC.make_case(n)[0]["q0"] + CC.make_case(n)[0]["dq"]
    t = lambda n: CC.make_case(n)[0]["t0"] + CC.make_case(n)[0]["dt"]
    assert 0.9 < q("benign").norm() < 1.1
    assert 7.5 < q("long_quaternion").norm() < 8.5
    assert 0.09 < q("short_quaternion").norm() < 0.11
    for k, axis in enumerate("xyz"):
        h = q("half_turn_" + axis)
        assert abs(h[0]) < 1e-3 and abs(h[1 + k]) > 0.9, (axis, h)
    ident = CC.make_case("identity")[0]
    assert ident["q0"].tolist() == [1.0, 0.0, 0.0, 0.0] and not ident["dq"].any()
    assert 990 < t("far_translation").norm() < 1010
    assert not t("zero_translation").any() and CC.make_case("zero_translation")[0]["t0"].any()
    fov = lambda n: (CC.make_case(n)[0]["fovx"].item(), CC.make_case(n)[0]["fovy"].item())
    assert fov("narrow_fov") == pytest.approx((0.05, 0.05), rel=1e-7)
    assert fov("wide_fov") == pytest.approx((2.8, 2.8), rel=1e-7)
    assert fov("unequal_fov") == pytest.approx((0.05, 2.8), rel=1e-7)
    nf = CC.make_case("near_far")[0]
    assert (nf["znear"], nf["zfar"]) == (0.5, 7.0)
    assert all((CC.make_case(n)[0]["znear"], CC.make_case(n)[0]["zfar"]) == (0.01, 100.0) for n in CC.CASES if n != "near_far")
    sk = CC.make_case("skewed_alignment")[0]
    assert abs(torch.linalg.det(sk["grot"]).item() - 1.0) > 0.1 and torch.linalg.cond(sk["grot"]).item() < 10
    assert (sk["grot"] @ sk["grot"].t() - torch.eye(3, dtype=torch.float64)).abs().max() > 0.1        # R^-1 is not R^T
    assert sk["gscale"].item() == pytest.approx(0.37, rel=1e-7)
    assert torch.linalg.det(CC.make_case("reflecting_alignment")[0]["grot"]).item() < -0.5
    ro, so, us = (CC.make_case(n)[0] for n in ("rotation_only", "scale_only", "unit_scale"))
    assert ro["grot"] is not None and ro["gscale"] is None
    assert so["grot"] is None and so["gscale"] is not None and so["gscale"].item() != 1.0
    assert us["gscale"].item() == 1.0 and (us["grot"] @ us["grot"].t() - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-6


def test_restated_intrinsic_is_the_projects_in_float32():
    """``_Chain.get_intrinsic`` (``projection_matrix`` without its float32 casts) gives ``PoseCamera.get_intrinsic``'s bits and
    gradients in float32, and stays float64 in float64; the inherited getters carry the dtype through."""
    for name in ("benign", "narrow_fov", "unequal_fov", "near_far"):
        inp, _ = CC.make_case(name)
        c = CC._Chain(inp, torch.float32)
        mine, theirs = c.get_intrinsic(), cam.PoseCamera.get_intrinsic(c)
        assert torch.equal(mine, theirs)
        k = torch.arange(16.0).reshape(4, 4) - 5.0
        a = torch.autograd.grad((mine * k).sum(), [c.learnable_fovx, c.learnable_fovy])
        b = torch.autograd.grad((theirs * k).sum(), [c.learnable_fovx, c.learnable_fovy])
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    inp, cots = CC.make_case("skewed_alignment")
    values, grads = CC.chain(inp, torch.float64, CC.ALL_ON, cots)
    assert all(v.dtype == torch.float64 for v in values.values()) and all(g.dtype == torch.float64 for g in grads.values())


@pytest.mark.parametrize("name", CC.CASES)
def test_chains_are_finite_and_float32_is_a_usable_yardstick(name):
    r = CC.reference(name)
    present = [n for n in CC.LEAVES if r["inputs"].get(n, 0) is not None]
    assert list(r["grads"]) == present
    for d in (r["values"], r["grads"], r["values32"], r["grads32"]):
        assert all(torch.isfinite(t).all() for t in d.values())
    for n in CC.VALUES:
        e, scale = r["err32"][0][n], r["values"][n].abs().max().item()
        print(f"{name} {n}: pytorch32 {e:.3e} (max-abs {scale:.3e})")
        assert math.isfinite(e) and e <= 1e-2 * scale, (n, e, scale)
    for n in present:
        e = r["err32"][1][n]
        print(f"{name} d{n}: pytorch32 {e:.3e}")
        assert e is not None and math.isfinite(e) and e < 1e-2, (n, e)       # under all four cotangents no gradient is zero
    vb, gb = r["bars"]
    assert all(vb[n] == max(4 * r["err32"][0][n], 16 * 2.0 ** -23 * r["values"][n].abs().max().item()) for n in CC.VALUES)
    assert all(gb[n] == max(4 * r["err32"][1][n], 16 * 2.0 ** -23) for n in present)


@pytest.mark.parametrize("name", NO_ALIGNMENT)
def test_float64_chain_is_a_camera(name):
    r = CC.reference(name)
    inp, v = r["inputs"], r["values"]
    V, M, K, C = (v[n] for n in CC.VALUES)
    R = V[:3, :3].t()                                                       # viewmatrix = W2C^T
    t = inp["t0"] + inp["dt"]
    assert (R @ R.t() - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-12
    assert torch.equal(V[3, :3], t) and torch.equal(V[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64))
    assert (C + R.t() @ t).abs().max() <= 1e-12 * max(1.0, t.abs().max().item())
    assert (M - V @ K).abs().max() <= 1e-12 * M.abs().max()
    assert K[0, 0].item() == pytest.approx(1.0 / math.tan(inp["fovx"].item() / 2), rel=1e-12)
    assert K[1, 1].item() == pytest.approx(1.0 / math.tan(inp["fovy"].item() / 2), rel=1e-12)
    assert K[2, 2].item() == pytest.approx(inp["zfar"] / (inp["zfar"] - inp["znear"]), rel=1e-12) and K[2, 3].item() == 1.0


def test_scale_only_is_a_scaled_translation():
    """csrc/camera.hip's header: scaling row 3 of inverse(W2C^T) by s and inverting back is t -> s t."""
    inp, _ = CC.make_case("scale_only")
    scaled, _ = CC.chain(inp, torch.float64)
    plain, _ = CC.chain(dict(inp, gscale=None), torch.float64)
    s = inp["gscale"]
    want = plain["viewmatrix"].clone()
    want[3, :3] *= s
    assert (scaled["viewmatrix"] - want).abs().max() < 1e-12
    assert (scaled["campos"] - s * plain["campos"]).abs().max() < 1e-12
    assert torch.equal(scaled["intrinsic"], plain["intrinsic"])


@pytest.mark.parametrize("name", ["benign", "skewed_alignment"])
@pytest.mark.parametrize("on", [CC.ALL_ON, (False, False, False, True), (False, True, False, False)])
def test_float64_gradients_are_central_differences(name, on):
    r = CC.reference(name, on)
    inp, cots = r["inputs"], r["cots"]

    def loss(x):
        v, _ = CC.chain(x, torch.float64)
        return sum((k * v[n]).sum().item() for k, n, use in zip(cots, CC.VALUES, on) if use)
    for leaf, g in r["grads"].items():
        fd = torch.zeros_like(g)
        for i in range(g.numel()):
            h = 1e-6 * max(1.0, abs(inp[leaf].reshape(-1)[i].item()))
            lo, hi = inp[leaf].clone(), inp[leaf].clone()
            lo.reshape(-1)[i] -= h
            hi.reshape(-1)[i] += h
            fd[i] = (loss(dict(inp, **{leaf: hi})) - loss(dict(inp, **{leaf: lo}))) / (2 * h)
        if g.norm() == 0:                                    # the fovs under the campos cotangent alone
            assert leaf in ("fovx", "fovy") and not on[1] and not on[2] and not fd.any()
            continue
        assert (fd - g).norm() <= 1e-6 * g.norm(), (leaf, fd, g)
