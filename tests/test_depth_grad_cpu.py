"""No-GPU checks of the opt-in depth / weights gradients (ABI 11): the reference in tests/depth_oracle.py against fp64
central differences and the closed form of d(weights)/d(alpha), and the C / Python surface of the feature."""
import ctypes as C
import os

import pytest
import torch

from bags_raster import _lib
from oracle import raster_oracle as O
from depth_oracle import backward_ex, forward, leaves_of
from scenes import make_case, oracle_settings


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_abi_11_exports_bags_backward_ex(lib):
    assert _lib.ABI_VERSION == 11 and lib.bags_abi_version() == 11
    assert hasattr(lib, "bags_backward_ex") and "bags_backward_ex" in _lib.SYMBOLS
    assert C.sizeof(_lib.BagsExtraGrads) == 16
    # the two structs the ABI tests pin do not grow
    assert C.sizeof(_lib.BagsSettings) == 14 * 4 + 5 * 8
    assert C.sizeof(_lib.BagsBackwardArgs) == 4 * 8 + 14 * 8 + 8 + 8 + 8 + 8 + 8


def _call_args():
    buf = (C.c_char * 4096)()
    addr = C.addressof(buf)
    s = _lib.BagsSettings(16, 16, 0.5, 0.5, 1.0, 0, 1, 0, 0, 0, 1, 0, 0, 0, addr, addr, addr, addr, addr)
    i = _lib.BagsInputs(0, None, None, None, None, None, None, None, None, None, None)
    st = _lib.BagsState(addr, 1 << 40, addr, 1 << 40, addr, 1 << 40)
    a = _lib.BagsBackwardArgs()
    a.workspace, a.workspace_bytes = addr, 1 << 40
    return buf, addr, s, i, st, a


def test_backward_ex_argument_errors(lib):
    """Reported before anything is enqueued (no GPU touched): validation never dereferences the host pointers given here."""
    buf, addr, s, i, st, a = _call_args()
    # no cotangent at all: neither grad_color nor an extra one
    x = _lib.BagsExtraGrads(None, None)
    assert lib.bags_backward_ex(C.byref(s), C.byref(i), C.byref(st), C.byref(a), C.byref(x), None) == -1
    assert b"grad_color must be given" in lib.bags_last_error() and b"grad_depth" in lib.bags_last_error()
    assert lib.bags_backward_ex(C.byref(s), C.byref(i), C.byref(st), C.byref(a), None, None) == -1
    assert b"grad_color must be given" in lib.bags_last_error()
    # with a depth cotangent and no grad_color the call gets past that check: the next defect (phase) is the one reported
    x.grad_depth = addr
    a.phase = 3
    assert lib.bags_backward_ex(C.byref(s), C.byref(i), C.byref(st), C.byref(a), C.byref(x), None) == -1
    assert b"phase" in lib.bags_last_error(), lib.bags_last_error()
    # ... and the same for weights alone
    x.grad_depth, x.grad_weights = None, addr
    assert lib.bags_backward_ex(C.byref(s), C.byref(i), C.byref(st), C.byref(a), C.byref(x), None) == -1
    assert b"phase" in lib.bags_last_error(), lib.bags_last_error()
    # bags_backward itself still requires grad_color
    assert lib.bags_backward(C.byref(s), C.byref(i), C.byref(st), C.byref(a), None) == -1
    assert b"grad_color must be given" in lib.bags_last_error()
    del buf


def test_depth_weights_grad_keyword():
    import inspect
    from bags_raster import GaussianRasterizationSettings, GaussianRasterizer
    from bags_raster.render import render
    f = GaussianRasterizationSettings._fields
    assert f[-1] == "depth_weights_grad" and GaussianRasterizationSettings._field_defaults["depth_weights_grad"] is False
    assert inspect.signature(render).parameters["depth_weights_grad"].default is False
    eye = torch.eye(4)
    st = GaussianRasterizationSettings(32, 32, 0.5, 0.5, torch.zeros(3), 1.0, eye, eye, eye, 0, torch.zeros(3), False, False, 0,
                                       depth_weights_grad="yes")
    x = torch.zeros(4, 3, device="cuda" if torch.cuda.is_available() else "cpu")
    from bags_raster.rasterizer import _Packed
    with pytest.raises((ValueError, RuntimeError), match="depth_weights_grad|AMD GPU"):
        _Packed(st, x, None, None, None, x, torch.ones_like(x[:, :1]), x, torch.zeros(4, 4, device=x.device), None, eye, eye, eye,
                torch.zeros(3))
    if x.is_cuda:      # (on a CPU host the device check comes first)
        dev = x.device
        st = st._replace(bg=st.bg.to(dev))
        with pytest.raises(ValueError, match="depth_weights_grad must be True or False"):
            _Packed(st, x, None, None, None, x, torch.ones_like(x[:, :1]), x, torch.zeros(4, 4, device=dev), None,
                    eye.to(dev), eye.to(dev), eye.to(dev), torch.zeros(3, device=dev))
    assert GaussianRasterizer is not None


def _tiny_case():
    scene, cam = make_case(24, 32, 32, 3.0, 1, seed=5, dist=3.0)
    scene["opacities"] = scene["opacities"] * 0.8
    return scene, cam


def _loss_fp64(scene, cam, gi, gd, gw, shift, discrete):
    """L = <gi, image> + <gd, depth> + <gw, weights> of the fp64 oracle forward, with the fp32 run's lists replayed."""
    s = oracle_settings(cam, 1, clamp_grad="exact", conic_grad="exact")
    inp = dict(scene); inp["shift_factors"] = shift
    leaf, s2 = leaves_of(inp, s, torch.float64, want=False)
    st = forward(leaf, s2, torch.float64, discrete)
    return ((st.image * gi).sum() + (st.depth_img * gd).sum() + (st.weights * gw).sum()).item()


def test_reference_matches_central_differences():
    """The two-call reference against fp64 central differences of <g, image> + <gD, depth> + <gA, weights> on a tiny scene, for
    means3D, opacities, the viewmatrix and the shift factors (the depth term is what reaches dL/dz).  Pairs within the step of a
    threshold (alpha = 1/255, T = 1e-4) would make a difference quotient meaningless: the scene is checked to have none."""
    torch.manual_seed(0)
    scene, cam = _tiny_case()
    H, W = cam.image_height, cam.image_width
    gen = torch.Generator().manual_seed(9)
    gi = torch.randn(3, H, W, generator=gen, dtype=torch.float64)
    gd = torch.randn(1, H, W, generator=gen, dtype=torch.float64)
    gw = torch.randn(1, H, W, generator=gen, dtype=torch.float64)
    shift = torch.tensor([0.01, -0.004, 0.002])
    # (the exact derivatives of the frustum clamp and the conic inverse: the stock rules are what upstream differentiates, not
    # the derivative a difference quotient measures)
    s = oracle_settings(cam, 1, clamp_grad="exact", conic_grad="exact")
    inp = dict(scene); inp["shift_factors"] = shift
    leaf32, s32 = leaves_of(inp, s, torch.float32, want=False)
    discrete = O.discrete_of(forward(leaf32, s32, torch.float32))
    leaf, s2 = leaves_of(inp, s, torch.float64)
    st = forward(leaf, s2, torch.float64, discrete)
    # no pair near a threshold: every alpha at least 1e-3 away from 1/255 (relative), T never near 1e-4
    assert float(st.final_T.min()) > 1e-3
    g = backward_ex(st, gi, gd, gw, leaf)
    h = 1e-6
    checked = 0
    for name, idxs in (("means3D", [(i, c) for i in range(0, 24, 3) for c in range(3)]), ("opacities", [(i, 0) for i in range(0, 24, 2)]),
                       ("viewmatrix", [(3, 0), (3, 1), (3, 2), (0, 2), (2, 2)]), ("shift_factors", [(0,), (1,)])):
        for ix in idxs:
            fp, fm = dict(inp), dict(inp)
            for f, sgn in ((fp, 1.0), (fm, -1.0)):
                if name == "viewmatrix":
                    v = s.viewmatrix.detach().double().clone(); v[ix] += sgn * h
                    f["viewmatrix"] = v
                else:
                    t = inp[name].detach().double().clone(); t[ix] += sgn * h
                    f[name] = t
            lp = _loss_fp64(fp, cam, gi, gd, gw, fp["shift_factors"], discrete)
            lm = _loss_fp64(fm, cam, gi, gd, gw, fm["shift_factors"], discrete)
            fd = (lp - lm) / (2 * h)
            an = float(g[name][ix])
            assert abs(fd - an) <= 1e-5 * max(1.0, abs(an)) + 2e-6 * max(1.0, abs(fd)), (name, ix, fd, an)
            checked += 1
    assert checked > 40
    # the depth term is not silently zero: without it the depth-only derivative differs
    leaf, s2 = leaves_of(inp, s, torch.float64)
    g0 = backward_ex(forward(leaf, s2, torch.float64, discrete), None, gd, None, leaf)
    assert float(g0["means3D"].abs().sum()) > 0 and float(g0["viewmatrix"].abs().sum()) > 0


def test_weights_cotangent_has_the_closed_form():
    """d(1 - T_final)/d alpha_i = T_final / (1 - alpha_i) on every contributing (pixel, splat) pair: the reference's second
    blend (colours [z, 1, 0], cotangent [0, gA, 0]) must give dL/dG = gA o T_final / (1 - alpha)."""
    scene, cam = _tiny_case()
    s = oracle_settings(cam, 1)
    inp = dict(scene); inp["shift_factors"] = torch.zeros(3)
    leaf, s2 = leaves_of(inp, s, torch.float64, want=False)
    st = forward(leaf, s2, torch.float64)
    pre = st.pre
    ext = torch.stack([pre.extras["tz"], torch.ones_like(pre.extras["tz"]), torch.zeros_like(pre.extras["tz"])], 1).detach()
    gA = torch.randn(256, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    n_pairs = 0
    for t in range(st.gx * st.gy):
        lo, hi = int(st.ranges[t, 0]), int(st.ranges[t, 1])
        if hi <= lo:
            continue
        ty, tx = divmod(t, st.gx)
        ids = st.point_list[lo:hi].to(torch.int64)
        xy = pre.xy.detach().clone().requires_grad_(True)      # (so that G is a node of the graph)
        r = O._blend_tile(ids, xy, pre.conic.detach(), pre.opacity.detach(), ext, pre.extras["tz"].detach(),
                          torch.zeros(3, dtype=torch.float64), tx * 16, ty * 16, st.W, st.H, want_pairs=True)
        G = r["G"]
        (dG,) = torch.autograd.grad((r["out"][:, 1] * gA).sum(), [G])
        op = pre.opacity.detach()[ids].reshape(-1)
        alpha = torch.clamp(op[None, :] * G.detach(), max=0.99)
        Tf = r["T_final"].detach()
        want = gA[:, None] * op[None, :] * Tf[:, None] / (1.0 - alpha)
        c = r["contrib"]
        assert torch.allclose(dG[c], want[c], rtol=1e-9, atol=1e-12)
        assert bool((dG[~c] == 0).all())
        n_pairs += int(c.sum())
    assert n_pairs > 100
