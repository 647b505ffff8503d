"""Fused pose -> matrix chain (csrc/camera.hip behind bags_camera_forward / bags_camera_backward) against the PyTorch chain
of bags_raster/camera.py, which tests/test_golden_cpu.py pins to the reference's getProjectionMatrix and
quaternion_to_rotation_matrix (scene/cameras.py:356-381,399-416; utils/graphics_utils.py:83-107), and, from
``test_chain_against_float64`` on, against the same chain in float64 at the edges of pose space (tests/camera_cases.py)."""
import functools
import itertools
from types import SimpleNamespace

import pytest
import torch

import camera_cases as CC
from bags_raster import _lib as L
from bags_raster import camera as cam

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _make(seed, device):
    g = torch.Generator().manual_seed(seed)
    R = cam.quaternion_to_rotation(torch.randn(4, generator=g))
    T = torch.randn(3, generator=g) + torch.tensor([0.0, 0.0, 4.0])
    c = cam.PoseCamera(R, T, 1.1, 0.7, 64, 48, device=device)
    with torch.no_grad():
        c.delta_quaternion.copy_(0.05 * torch.randn(4, generator=g))
        c.delta_translation.copy_(0.1 * torch.randn(3, 1, generator=g))
        c.learnable_fovx.add_(0.03); c.learnable_fovy.sub_(0.02)
    return c


@pytest.mark.parametrize("align", [False, True])
def test_fused_camera_chain_matches_pytorch_chain(align):
    g = torch.Generator().manual_seed(9)
    grot = cam.quaternion_to_rotation(torch.tensor([1.0, 0.02, -0.03, 0.01])) if align else None
    gscale = torch.tensor(1.3) if align else None
    cots = [torch.randn(4, 4, generator=g), torch.randn(4, 4, generator=g), torch.randn(4, 4, generator=g), torch.randn(3, generator=g)]
    # reference chain on the CPU in float64-free plain float32 PyTorch
    c0 = _make(4, "cpu")
    gr0 = None if grot is None else grot.clone().requires_grad_(True)
    gs0 = None if gscale is None else gscale.clone().requires_grad_(True)
    want = c0.get_matrices(gr0, gs0)
    loss = sum((w * k).sum() for w, k in zip(want, cots))
    leaves0 = c0.pose_leaves() + ([gr0, gs0] if align else [])
    gwant = torch.autograd.grad(loss, leaves0)
    # fused chain on the GPU
    c1 = _make(4, DEV)
    gr1 = None if grot is None else grot.to(DEV).requires_grad_(True)
    gs1 = None if gscale is None else gscale.to(DEV).requires_grad_(True)
    got = c1.get_matrices(gr1, gs1)
    for a, b in zip(got, want):
        assert torch.allclose(a.cpu(), b.detach(), rtol=1e-5, atol=2e-6), (a.cpu() - b.detach()).abs().max()
    loss = sum((w * k.to(DEV)).sum() for w, k in zip(got, cots))
    leaves1 = c1.pose_leaves() + ([gr1, gs1] if align else [])
    ggot = torch.autograd.grad(loss, leaves1)
    for a, b in zip(ggot, gwant):
        assert a.shape == b.shape
        assert torch.allclose(a.cpu(), b, rtol=2e-4, atol=2e-5), (a.cpu(), b)


def test_fused_camera_chain_partial_gradients_and_errors():
    c = _make(5, DEV)
    V, M, K, C = c.get_matrices()
    (gq,) = torch.autograd.grad(C.sum(), [c.delta_quaternion], retain_graph=True)      # only one leaf, only campos upstream
    assert torch.isfinite(gq).all() and gq.abs().sum() > 0
    (gf,) = torch.autograd.grad(K[0, 0], [c.learnable_fovx])
    t = torch.tan(c.learnable_fovx.detach() * 0.5)
    assert abs(gf.item() - (-(1 + t * t) / (2 * t * t)).item()) < 1e-4
    with pytest.raises(RuntimeError, match="GPU"):
        cam.fused_camera_chain(torch.zeros(4), torch.zeros(3), torch.tensor(1.0), torch.tensor(1.0), torch.tensor([1.0, 0, 0, 0]), torch.zeros(3))


def test_render_uses_fused_chain_and_reaches_pose_leaves():
    """render() -> PoseCamera.get_matrices -> HIP camera chain -> rasterizer; gradients arrive on the four pose leaves and
    agree with the same render driven by the PyTorch chain."""
    from bags_raster.gaussians import GaussianBag
    from bags_raster.render import render, PipelineParams
    from bags_raster.synth import synth_scene, sphere_views
    scene = synth_scene(1200, 5, 1.5, 3)
    W, H = 128, 96
    gimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(2)).to(DEV)

    class Plain:                                   # hides get_matrices: render() falls back to the four getters
        def __init__(self, c): self.c = c
        def __getattr__(self, k):
            if k == "get_matrices":
                raise AttributeError(k)
            return getattr(self.c, k)
    res = []
    for wrap in (lambda c: c, Plain):
        c = sphere_views(2, W, H, noise=0.05, device=DEV)[1]
        pc = GaussianBag.from_activated(scene, 3, device=DEV)
        out = render(wrap(c), pc, PipelineParams(), torch.zeros(3, device=DEV), 0.0, None, hybrid=False)
        out["render"].backward(gimg)
        res.append((out["render"].detach().cpu(), [p.grad.detach().cpu().clone() for p in c.pose_leaves()]))
    assert (res[0][0] - res[1][0]).abs().max().item() < 2e-4
    for a, b in zip(res[0][1], res[1][1]):
        assert (a - b).norm().item() <= 2e-3 * b.norm().item() + 1e-6, (a, b)


def test_fused_camera_chain_matches_reference_methods(golden_dir):
    """csrc/camera.hip against tests/golden/camera_pose_chain.npz: the values and Jacobians the reference's own Camera methods
    (scene/cameras.py:356-381, run on a stub self by make_golden.py) produce, with and without global alignment."""
    import os
    import numpy as np
    g = np.load(os.path.join(golden_dir, "camera_pose_chain.npz"))
    rs = np.random.RandomState(0)
    for i in range(g["x"].shape[0]):
        x = torch.tensor(g["x"][i], device=DEV)
        leaves = [x[0:4].clone().requires_grad_(True), x[4:7].clone().view(3, 1).requires_grad_(True), x[7].clone().requires_grad_(True),
                  x[8].clone().requires_grad_(True), x[9:18].clone().view(3, 3).requires_grad_(True), x[18:19].clone().requires_grad_(True)]
        q0 = torch.tensor(g["init_quaternion"][i], device=DEV); t0 = torch.tensor(g["init_translation"][i], device=DEV)
        V, M, K, C = cam.fused_camera_chain(leaves[0], leaves[1], leaves[2], leaves[3], q0, t0, 0.01, 100.0, leaves[4], leaves[5])
        y = torch.cat([V.reshape(-1), M.reshape(-1), K.reshape(-1), C.reshape(-1)])
        assert np.allclose(y.detach().cpu().numpy(), g["y"][i], rtol=2e-5, atol=2e-6), np.abs(y.detach().cpu().numpy() - g["y"][i]).max()
        J = g["dy_dx"][i].astype(np.float64)
        for _ in range(4):                                    # vector-Jacobian products with random cotangents
            c = rs.randn(51)
            gs = torch.autograd.grad(y, leaves, torch.tensor(c, dtype=torch.float32, device=DEV), retain_graph=True)
            got = torch.cat([a.reshape(-1) for a in gs]).cpu().numpy().astype(np.float64)
            want = c @ J
            assert np.abs(got - want).max() <= 3e-4 * np.abs(want).max() + 1e-5, (i, np.abs(got - want).max(), np.abs(want).max())
        if i < 2:                                             # no alignment: the None / None call gives the same four tensors
            V0, M0, K0, C0 = cam.fused_camera_chain(leaves[0], leaves[1], leaves[2], leaves[3], q0, t0)
            y0 = torch.cat([V0.reshape(-1), M0.reshape(-1), K0.reshape(-1), C0.reshape(-1)])
            assert np.allclose(y0.detach().cpu().numpy(), g["y"][i], rtol=2e-5, atol=2e-6)


# --------------------------------------------------------------------------------------------- the float64 rule (tests/camera_cases.py)
# The kernel's error against the float64 chain is at most FACTOR x the float32 PyTorch chain's own error on the same input, floored at
# 16 float32 epsilons; the cases, the reference and the bar are checked on the CPU by tests/test_camera_cases_cpu.py.
SUBSETS = [on for on in itertools.product((False, True), repeat=4) if any(on)]          # the 15 non-empty subsets of {gV, gM, gK, gC}
GRADS = ("dq", "dt", "fovx", "fovy", "grot", "gscale")


def _device_inputs(name):
    """The float32 cast of a case on the GPU: dict of fresh tensors in the shapes ``PoseCamera`` keeps (dt and t0 (3,1)), and the cotangents."""
    inp, cots = CC.make_case(name)
    f = lambda t: None if t is None else t.to(torch.float32).to(DEV)
    d = {k: (v if isinstance(v, float) else f(v)) for k, v in inp.items()}
    d["t0"], d["dt"] = d["t0"].reshape(3, 1), d["dt"].reshape(3, 1)
    return d, [f(c) for c in cots]


def _run(d, cots, wanted=GRADS, on=CC.ALL_ON):
    """fused_camera_chain and one backward of ``sum_i <cots[i], out_i>`` over the cotangents switched ``on``; only the leaves named in
    ``wanted`` require a gradient.  Returns (values by name, gradients by name with None for a leaf that got none, the four outputs,
    the leaves)."""
    leaves = {n: (None if d[n] is None else d[n].detach().requires_grad_(n in wanted)) for n in GRADS}      # detach: the strides stay
    out = cam.fused_camera_chain(leaves["dq"], leaves["dt"], leaves["fovx"], leaves["fovy"], d["q0"], d["t0"], d["znear"], d["zfar"],
                                 leaves["grot"], leaves["gscale"])
    loss = sum((k * o).sum() for k, o, use in zip(cots, out, on) if use)
    asked = [n for n in GRADS if leaves[n] is not None and leaves[n].requires_grad]
    gs = torch.autograd.grad(loss, [leaves[n] for n in asked], retain_graph=True, allow_unused=True)
    grads = {n: None for n in GRADS}
    grads.update(zip(asked, gs))
    return {n: o.detach() for n, o in zip(CC.VALUES, out)}, grads, out, leaves


@functools.lru_cache(maxsize=None)
def _all_six(name):
    d, cots = _device_inputs(name)
    values, grads, _, _ = _run(d, cots)
    return d, cots, values, grads


def _assert_meets_bars(tag, ref, values, grads):
    """``values`` / ``grads`` (GPU tensors by name; either may be None) against ``CC.reference``'s float64 chain, printing the margins."""
    vb, gb = ref["bars"]
    for n in (values or {}):
        e, e32 = CC.value_error(values[n].cpu(), ref["values"][n]), ref["err32"][0][n]
        print(f"{tag} {n}: kernel {e:.3e} pytorch32 {e32:.3e}")
        assert e <= vb[n], (tag, n, e, e32, vb[n])
    for n in (grads or {}):
        if n not in ref["grads"]:                            # an absent alignment input
            assert grads[n] is None, (tag, n)
            continue
        got = grads[n].cpu()
        e, e32 = CC.gradient_error(got, ref["grads"][n]), ref["err32"][1][n]
        if e is None:                                        # the float64 gradient is identically zero: exact zeros
            assert not got.any(), (tag, n, got)
            continue
        print(f"{tag} d{n}: kernel {e:.3e} pytorch32 {e32:.3e}")
        assert e <= gb[n], (tag, n, e, e32, gb[n])


@pytest.mark.parametrize("name", CC.CASES)
def test_chain_against_float64(name):
    d, cots, values, grads = _all_six(name)
    ref = CC.reference(name)
    assert all((grads[n] is None) == (d[n] is None) for n in GRADS)
    assert all(grads[n].shape == d[n].shape for n in GRADS if d[n] is not None)
    _assert_meets_bars(name, ref, values, grads)


def _c_backward(d, cots, null=True, wanted=GRADS):
    """``bags_camera_backward`` itself, as ``_FusedCameraChain.backward`` calls it, but with real NULLs (``null``) or zero-filled
    tensors (the wrapper's route) for the absent cotangents.  Returns the gradients by name (None where none was asked for or the
    alignment input is absent)."""
    keep = {n: None if d[n] is None else L.as_f32c(d[n]).reshape(-1) for n in ("q0", "dq", "t0", "dt", "fovx", "fovy", "grot", "gscale")}
    camera = L.BagsCamera(*[L.ptr(keep[n]) for n in ("q0", "dq", "t0", "dt", "fovx", "fovy", "grot", "gscale")], float(d["znear"]), float(d["zfar"]))
    shapes = ((4, 4), (4, 4), (4, 4), (3,))
    given = [None if c is None else L.as_f32c(c) for c in cots]
    if not null:
        given = [torch.zeros(s, dtype=torch.float32, device=DEV) if c is None else c for c, s in zip(given, shapes)]
    assert all(c is None or (c.shape == s and c.is_cuda) for c, s in zip(given, shapes))
    sizes = dict(dq=4, dt=3, fovx=1, fovy=1, grot=9, gscale=1)
    out = {n: torch.full((sizes[n],), float("nan"), dtype=torch.float32, device=DEV) if (n in wanted and d[n] is not None) else None for n in GRADS}
    L.call("bags_camera_backward", d["dq"].device, camera, *[L.ptr(c) for c in given], *[L.ptr(out[n]) for n in GRADS])
    return out


@pytest.mark.parametrize("on", SUBSETS, ids=lambda on: "".join(c for c, use in zip("VMKC", on) if use))
@pytest.mark.parametrize("name", ["benign", "skewed_alignment"])
def test_cotangent_subsets(name, on):
    """The kernel's null-cotangent branches, which autograd never reaches (it hands zero-filled tensors over): through the C entry."""
    d, cots = _device_inputs(name)
    some = [c if use else None for c, use in zip(cots, on)]
    nulls = _c_backward(d, some, null=True)
    zeros = _c_backward(d, some, null=False)
    ref = CC.reference(name, on)
    tag = f"{name} " + "".join(c for c, use in zip("VMKC", on) if use)
    _assert_meets_bars(tag, ref, None, nulls)
    for n in GRADS:
        assert torch.equal(nulls[n], zeros[n]), (tag, n, nulls[n], zeros[n])
    if not (on[1] or on[2]):                                 # the fovs are reached through intrinsic and projmatrix alone
        assert not ref["grads"]["fovx"].any() and not ref["grads"]["fovy"].any()
        assert not nulls["fovx"].any() and not nulls["fovy"].any()
    if on == CC.ALL_ON:                                      # the entry called directly is the wrapper's call
        for n in GRADS:
            assert torch.equal(nulls[n], _all_six(name)[3][n].reshape(-1)), (tag, n)


@pytest.mark.parametrize("wanted", [("dq",), ("dt",), ("fovx",), ("fovy",), ("grot",), ("gscale",), ("dq", "dt"), ("fovx", "fovy")], ids="+".join)
@pytest.mark.parametrize("name", ["benign", "skewed_alignment"])
def test_gradient_subsets(name, wanted, monkeypatch):
    """Frozen leaves: the wrapper passes NULL for their gradients, the others keep the bits of the all-six run."""
    d, cots, _, full = _all_six(name)
    passed = []
    real_call = L.call

    def spying_call(entry, device, *args):
        if entry == "bags_camera_backward":
            passed.append(args[5:11])
        return real_call(entry, device, *args)
    monkeypatch.setattr(L, "call", spying_call)
    _, grads, _, leaves = _run(d, cots, wanted=wanted)
    assert len(passed) == 1
    assert [p is not None for p in passed[0]] == [n in wanted for n in GRADS], passed       # NULL for every gradient not asked for
    for n in GRADS:
        if n in wanted:
            assert grads[n].shape == d[n].shape and torch.equal(grads[n], full[n]), (n, grads[n], full[n])
        else:
            assert grads[n] is None and leaves[n].grad is None, n


@pytest.mark.parametrize("name", ["benign", "skewed_alignment"])
def test_gradient_subsets_without_alignment(name):
    """``_FusedCameraChain.backward`` returns None for g_grot / g_gscale when that input is absent, even when told they are needed,
    and for every leaf it is told is not needed."""
    d, cots, _, full = _all_six(name)
    for drop in (("grot",), ("gscale",), ("grot", "gscale")):
        ctx = SimpleNamespace()
        dd = {k: (None if k in drop else v) for k, v in d.items()}
        cam._FusedCameraChain.forward(ctx, dd["dq"], dd["dt"], dd["fovx"], dd["fovy"], dd["q0"], dd["t0"], dd["znear"], dd["zfar"], dd["grot"], dd["gscale"])
        ctx.needs_input_grad = (True,) * 10
        r = cam._FusedCameraChain.backward(ctx, *cots)
        assert len(r) == 10 and all(r[k] is None for k in (4, 5, 6, 7))
        for k, n in zip((0, 1, 2, 3, 8, 9), GRADS):
            assert (r[k] is None) == (n in drop), (drop, n)
        # the same call through autograd
        _, grads, _, _ = _run(dd, cots)
        for k, n in zip((0, 1, 2, 3, 8, 9), GRADS):
            assert (grads[n] is None and r[k] is None) or torch.equal(grads[n], r[k]), (drop, n)
        ctx.needs_input_grad = (False, True) + (False,) * 8
        r = cam._FusedCameraChain.backward(ctx, *cots)
        assert [x is not None for x in r] == [k == 1 for k in range(10)]
        assert torch.equal(r[1], grads["dt"])


def test_backward_twice_and_on_a_side_stream():
    for name in ("benign", "skewed_alignment"):
        d, cots, values, full = _all_six(name)
        _, first, out, leaves = _run(d, cots)
        loss = sum((k * o).sum() for k, o in zip(cots, out))
        second = torch.autograd.grad(loss, [leaves[n] for n in GRADS])                          # the retained graph again
        for n, g in zip(GRADS, second):
            assert torch.equal(first[n], g) and torch.equal(full[n], g), n
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            v_side, g_side, _, _ = _run(d, cots)
        side.synchronize()
        torch.cuda.current_stream().wait_stream(side)
        for n in CC.VALUES:
            assert torch.equal(v_side[n], values[n]), n
        for n in GRADS:
            assert torch.equal(g_side[n], full[n]), n


def test_non_contiguous_and_shaped_leaves():
    d, cots, values, full = _all_six("benign")
    ref = CC.reference("benign")
    flat = d["dt"].reshape(3)
    strided = torch.zeros(6, device=DEV)
    strided[::2] = flat
    for dt in (d["dt"].reshape(3, 1), flat, strided[::2]):
        v, g, _, _ = _run(dict(d, dt=dt), cots)
        assert g["dt"].shape == dt.shape
        _assert_meets_bars(f"benign dt{tuple(dt.shape)}/{dt.stride()}", ref, v, g)
        assert all(torch.equal(v[n], values[n]) for n in CC.VALUES)
        assert all(torch.equal(g[n].reshape(-1), full[n].reshape(-1)) for n in GRADS)
    # grot as a transposed, non-contiguous view of a leaf: the gradient arrives on the leaf, in its shape, transposed
    base = d["grot"].t().contiguous().requires_grad_(True)
    assert not base.t().is_contiguous()
    out = cam.fused_camera_chain(d["dq"], d["dt"], d["fovx"], d["fovy"], d["q0"], d["t0"], d["znear"], d["zfar"], base.t(), d["gscale"])
    assert all(torch.equal(o, values[n]) for o, n in zip(out, CC.VALUES))
    sum((k * o).sum() for k, o in zip(cots, out)).backward()
    assert base.grad.shape == (3, 3) and torch.equal(base.grad.t(), full["grot"])
    _assert_meets_bars("benign grot.t()", ref, {n: o.detach() for n, o in zip(CC.VALUES, out)}, dict(grot=base.grad.t()))
    # wrong element counts
    five, four, eight = torch.zeros(5, device=DEV), torch.zeros(4, device=DEV), torch.zeros(8, device=DEV)
    for bad, n in ((dict(dq=five), 4), (dict(dt=four), 3), (dict(grot=eight), 9), (dict(q0=five), 4), (dict(fovx=four[:2]), 1), (dict(gscale=four[:2]), 1)):
        b = dict(d, **bad)
        with pytest.raises(RuntimeError, match=f"expected {n} values, got {next(iter(bad.values())).numel()}"):
            cam.fused_camera_chain(b["dq"], b["dt"], b["fovx"], b["fovy"], b["q0"], b["t0"], b["znear"], b["zfar"], b["grot"], b["gscale"])
