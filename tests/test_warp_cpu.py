"""No-GPU checks of the warping loss (bags_raster/warp.py, csrc/warp.hip): gradcheck of the PyTorch statement, the statement against
the closed forms, that the bars of tests/warp_cases.py reject wrong answers, the generator's conditions, the degenerate pairs in
float64, warp_image_torch against grid_sample, two identical views, a pose perturbation against a finite difference, the C surface
and the rejections of its entry points and of the Python wrappers."""
import ctypes as C
import math
import os

import pytest
import torch

import warp_cases as P
import bags_raster
from bags_raster import _lib, warp_image, warp_image_torch, warp_loss, warp_loss_torch

FUNCS = ("bags_warp_workspace_size", "bags_warp_forward", "bags_warp_backward", "bags_warp_image")
PUBLIC = ("warp_loss", "warp_loss_torch", "warp_image", "warp_image_torch")
F64 = torch.float64
IDS = ["%dx%d" % s for s in P.SHAPES]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _pair(c, k, dtype=F64):
    """The arguments of one pair of a case for the statement, in ``dtype``."""
    maps = (c["D_dst"][k].to(dtype), c["A_dst"][k].to(dtype)) if bool(c["has_dst"][k]) else (None, None)
    return dict(args=(c["D"][k].to(dtype), c["A"][k].to(dtype), c["Vi"][k].to(dtype), c["Vj"][k].to(dtype), c["color"][k].to(dtype), c["image"][k].to(dtype),
                      c["pin_i"][k], c["pin_j"][k], c["conf"][k].to(dtype)) + maps,
                kw=dict(eps=c["eps"], occlusion=P.OCCLUSION, min_weight=P.MIN_WEIGHT, min_depth=P.MIN_DEPTH))


# ---------------------------------------------------------------------------------------------------------------- the function
def _round_off(a, b, s):
    """|a - b| within float64 round-off of the sum of the absolute values of the terms ``s``, element by element; exact where ``s`` is 0.
    The residual r = S - color_src is itself a difference of two numbers of order 1, which ``s`` does not see: where the colour noise
    is 1e-4 the gradient carries that cancellation, hence the second term, from the largest element."""
    return bool(((a - b).abs() <= torch.where(s > 0, 1e-10 * s + 1e-12 * s.max(), torch.zeros_like(s))).all())


@pytest.mark.parametrize("eps", P.EPSES)
@pytest.mark.parametrize("channels", P.CHANNELS)
def test_gradcheck_of_the_statement(channels, eps):
    c = P.make_case(3, 5, 2, channels, eps)
    for k in range(2):                                       # with target maps and without
        p = _pair(c, k)
        leaf = lambda t: t.clone().requires_grad_(True)                                  # noqa: E731
        D, A, Vi, Vj = (leaf(t) for t in p["args"][:4])
        f = lambda D, A, Vi, Vj: warp_loss_torch(D, A, Vi, Vj, *p["args"][4:], **p["kw"])[0]              # noqa: E731
        assert f(D, A, Vi, Vj).item() > 0
        assert torch.autograd.gradcheck(f, (D, A, Vi, Vj))


@pytest.mark.parametrize("eps", P.EPSES)
@pytest.mark.parametrize("channels", P.CHANNELS)
@pytest.mark.parametrize("H,W", P.SHAPES, ids=IDS)
def test_statement_equals_the_closed_forms(H, W, channels, eps):
    """warp_loss_torch in float64 with autograd against the closed forms of the loss and of the four gradients, element by element to
    round-off; exact zeros where the closed form has zeros (invalid pixels, the fourth columns)."""
    for K in (2, 17):
        c = P.make_case(H, W, K, channels, eps)
        ref, want = P.reference(H, W, K, channels, eps), P.closed_form(c)
        for name, a, b, s in zip(P.NAMES, ref[:5], want, P.scales(c)):
            assert a.shape == b.shape and torch.isfinite(a).all(), name
            assert _round_off(a, b, s), (name, float(((a - b).abs() / s.clamp_min(1e-300)).max()))
            assert bool(((b == 0) <= (a == 0)).all()), name
        assert (ref[5] - P._pieces(c)["cnt"]).abs().max() < 1e-12
        assert (ref[0] > 0).all() and (ref[5] > 0).all() and all(t.abs().max() > 0 for t in ref[1:5])
        assert ref[3][:, :, 3].abs().max() == 0 and ref[4][:, :, 3].abs().max() == 0


def test_bars_reject_wrong_answers():
    """The closed forms are far inside the bars on every case; each of the four wrong answers -- the sample taken at proj + 0.5, dS/dproj
    with ax and ay exchanged, the 1/C missing from the gradient, the L1 gradient sign(r) -- is outside every gradient's bar on every
    case (the missing 1/C on every case of three channels; with one channel it is no error)."""
    for H, W in P.SHAPES:
        for K in P.PAIRS:
            for channels in P.CHANNELS:
                for eps in P.EPSES:
                    key = (H, W, K, channels, eps)
                    c = P.make_case(*key)
                    good = P.margins(*key, P.closed_form(c))
                    assert all(m <= 1e-3 for m in good), (key, good)
                    m = P.margins(*key, P.closed_form(c, half_pixel=True))
                    assert all(x > 1.0 for x in m), ("half_pixel", key, m)
                    m = P.margins(*key, P.closed_form(c, swap_ax_ay=True))
                    assert m[0] <= 1e-3 and all(x > 1.0 for x in m[1:]), ("swap_ax_ay", key, m)
                    m = P.margins(*key, P.closed_form(c, drop_one_over_c=True))
                    assert m[0] <= 1e-3 and all((x > 1.0) == (channels == 3) for x in m[1:]), ("drop_one_over_c", key, m)
                    m = P.margins(*key, P.closed_form(c, l1_gradient=True))
                    assert m[0] <= 1e-3 and all(x > 1.0 for x in m[1:]), ("l1_gradient", key, m)


def test_generator_conditions_hold_on_every_case():
    worst = dict(gap=1.0, front=1.0, valid=1.0, outside=1.0)
    guard, cell, inside, occluded = 0.0, [1.0, 0.0], [1.0, 0.0], [1.0, 0.0]
    for H, W in P.SHAPES:
        for K in P.PAIRS:
            for channels in P.CHANNELS:
                for eps in P.EPSES:
                    f = P.check_case(P.make_case(H, W, K, channels, eps))
                    for k in ("gap", "front", "valid"):
                        worst[k] = min(worst[k], f[k])
                    guard = max(guard, f["guard"])
                    if H * W >= P.SMALL:
                        worst["outside"] = min(worst["outside"], f["outside"])
                        for acc, name in ((cell, "cell"), (inside, "inside"), (occluded, "occluded")):
                            acc[0], acc[1] = min(acc[0], f[name][0]), max(acc[1], f[name][1])
    for channels in P.CHANNELS:
        for eps in P.EPSES:
            P.check_case(P.degenerate_case(channels, eps))
    print("\nwarp cases: smallest |A - min_weight| %.3g, |x_j.z - min_depth| %.3g, valid share %.3f; inside %.3f .. %.3f of all pixels, outside "
          "at least %.3f of the projected ones, occluded %.3f .. %.3f of the inside ones; guards at most %.4f of a pair's pixels, the cell-line "
          "guard alone %.4f .. %.4f" % (worst["gap"], worst["front"], worst["valid"], inside[0], inside[1], worst["outside"], occluded[0],
                                        occluded[1], guard, cell[0], cell[1]))
    assert worst["valid"] >= 0.5 and guard <= 0.03 and worst["outside"] >= 0.17 and 0.10 <= occluded[0] and occluded[1] <= 0.20
    assert P.SEAM[0] * P.SEAM[1] > 2 * P.CHUNK and (P.SEAM[0] * P.SEAM[1]) % P.CHUNK != 0
    a, b = P.make_case(17, 67, 2, 3, 1e-3), P.make_case(17, 67, 2, 1, 0.1)
    assert a is P.make_case(17, 67, 2, 3, 1e-3)                                           # cached, shared
    assert torch.equal(a["D"], b["D"]) and torch.equal(a["image"][:, :1].nan_to_num(7.0), b["image"].nan_to_num(7.0)) and torch.equal(a["conf"], b["conf"])       # one scene for every C and eps
    assert (a["Hd"], a["Wd"]) != (a["H"], a["W"]) and not bool(a["has_dst"][1]) and bool(a["has_dst"][0])
    assert (a["pin_i"] - a["pin_j"]).abs().min() > 0                                       # different pinholes on the two sides


@pytest.mark.parametrize("eps", P.EPSES)
@pytest.mark.parametrize("channels", P.CHANNELS)
def test_degenerate_pairs_give_zero_loss_and_zero_gradients(channels, eps):
    c = P.degenerate_case(channels, eps)
    assert len(c["degenerate"]) == 6
    for dtype in (F64, torch.float32):
        res = P.run_torch(c, dtype)
        assert all(torch.isfinite(t).all() for t in res)
        for k in c["degenerate"]:
            assert res[0][k] == 0 and res[5][k] == 0 and all(res[i][k].abs().max() == 0 for i in (1, 2, 3, 4)), (dtype, k)
        keep = [k for k in range(16) if k not in c["degenerate"]]
        assert (res[0][keep] > 0).all() and (res[5][keep] > 0).all()
    want = P.closed_form(c)
    for name, a, b, s in zip(P.NAMES, P.run_torch(c, F64)[:5], want, P.scales(c)):
        assert _round_off(a, b, s), name
    assert all(s[k].abs().max() == 0 for s in P.scales(c) for k in c["degenerate"])      # their bars are 0: exact zeros


@pytest.mark.parametrize("H,W", ((3, 5), (17, 67), P.SEAM), ids=("3x5", "17x67", "seam"))
def test_warp_image_torch_is_grid_sample_with_align_corners(H, W):
    """Both put pixel centres at whole numbers, so only the normalisation of the coordinates differs: on the valid pixels the warped
    image is F.grid_sample(image_dst, bilinear, align_corners=True) at proj."""
    c = P.make_case(H, W, 2, 3, 1e-3)
    q = P._pieces(c)
    for k in range(2):
        p = _pair(c, k)["args"]
        img = torch.nan_to_num(p[5], nan=0.25)                                            # grid_sample spreads a NaN texel differently
        out, valid = warp_image_torch(p[0], p[1], p[2], p[3], img, p[6], p[7], p[9], p[10], occlusion=P.OCCLUSION)
        assert out.dtype == F64 and tuple(out.shape) == (3, H, W) and valid.dtype == torch.bool and tuple(valid.shape) == (H, W)
        assert torch.equal(valid, q["inside"][k] & q["visible"][k]) and valid.any()
        assert out[:, ~valid].abs().max() == 0 if (~valid).any() else True
        grid = torch.stack([2 * q["x"][k] / (c["Wd"] - 1) - 1, 2 * q["y"][k] / (c["Hd"] - 1) - 1], -1)[None]
        want = torch.nn.functional.grid_sample(img[None], grid, mode="bilinear", padding_mode="border", align_corners=True)[0]
        assert (out - want)[:, valid].abs().max() <= 1e-12


def _wall(H=12, W=16, z0=2.5):
    """A textured wall at depth z0 in front of a camera: maps, pinhole, an image of periods of about 8 pixels."""
    A = torch.full((1, H, W), 0.8125, dtype=F64)
    y, x = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    img = torch.stack([0.5 + 0.4 * torch.sin(0.8 * x + 0.3 * c) * torch.cos(0.7 * y - 0.2 * c) for c in range(3)])
    return A * z0, A, (14.0, 13.0, 7.25, 5.5), img


def test_two_identical_views_have_zero_loss():
    """A pair of a view with itself and color_src = image_dst: proj is the pixel itself up to round-off, so S = color_src up to
    round-off times the texture's slope and rho = sqrt(r^2 + eps^2) - eps = r^2 / (2 eps) or so."""
    D, A, pin, img = _wall()
    V = torch.eye(4, dtype=F64)
    V[:3, :3] = 1.3 * P.so3_exp(torch.tensor((0.2, -0.1, 0.3))).double()
    V[3, :3] = torch.tensor((0.1, -0.2, 0.3), dtype=F64)
    for eps in P.EPSES:
        loss, count = warp_loss_torch(D, A, V, V, img, img, pin, pin, depth_dst=D, weights_dst=A, eps=eps)
        # (a border pixel whose proj comes out a rounding error outside [0, W - 1] is outside: inside is a decision on proj as computed)
        assert 10 * 14 <= count.item() <= D.numel() and 0 <= loss.item() <= (1e-12) ** 2 / eps
    assert warp_loss_torch(D, A, V, V, img[:1], img[:1], pin, pin)[0].item() <= 1e-21      # one channel


def test_a_pose_perturbation_gives_a_positive_loss_and_the_gradient_of_a_finite_difference():
    D, A, pin, img = _wall()
    Vi, Vj = torch.eye(4, dtype=F64), torch.eye(4, dtype=F64)
    Vj[:3, :3] = P.so3_exp(torch.tensor((0.004, -0.006, 0.003))).double()
    Vj[3, :3] = torch.tensor((0.05, -0.03, 0.02), dtype=F64)
    f = lambda Vj: warp_loss_torch(D, A, Vi, Vj, img, img, pin, pin, eps=0.1)[0].sum()   # noqa: E731
    assert f(Vi).item() <= 1e-21
    leaf = Vj.clone().requires_grad_(True)
    loss = f(leaf)
    assert loss.item() > 1e-4
    g, = torch.autograd.grad(loss, leaf)
    assert g[:, 3].abs().max() == 0
    h, checked = 1e-6, 0
    for r in range(4):
        for k in range(3):
            step = torch.zeros(4, 4, dtype=F64)
            step[r, k] = h
            fd = (f(Vj + step) - f(Vj - step)).item() / (2 * h)
            if abs(fd) > 1e-4:                                # (no projection crosses a cell line over 1e-6: the loss is smooth there)
                assert g[r, k].item() * fd > 0 and abs(g[r, k].item() - fd) <= 1e-4 * abs(fd), (r, k, g[r, k].item(), fd)
                checked += 1
    assert checked >= 6


# ---------------------------------------------------------------------------------------------------------------- the surface
def test_public_names_and_c_surface(lib):
    for name in PUBLIC:
        assert getattr(bags_raster, name) is not None and name in bags_raster.__all__, name
    for name in FUNCS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 11 and lib.bags_abi_version() == 11
    assert C.sizeof(_lib.BagsWarp) == 16 + 8 + 16 + 2 * 8 + 2 * 16 * 4 * 8 + 9 * 16 * 8
    assert _lib.BagsWarp.eps.offset == 40 and _lib.BagsWarp.pinhole_src.offset == 56 and _lib.BagsWarp.depth.offset == 56 + 1024
    size, co = lib.bags_warp_workspace_size, lib.bags_correspondence_workspace_size
    chunks = lambda H, W: -(-H * W // 256)                                               # noqa: E731
    assert 12 * 8 <= size(1, 1, 1) <= 256 and size(16, 1080, 1920) == 16 * chunks(1080, 1920) * 12 * 8 and 3 * 3 * 12 * 8 <= size(3, 7, 92) <= 1024
    assert all(size(n, H, W) == co(n, H, W) for n, H, W in ((1, 1, 1), (3, 7, 92), (16, 1080, 1920)))        # the rows of the correspondence loss
    assert size(0, 4, 4) == 0 and size(17, 4, 4) == 0 and size(1, 0, 4) == 0 and size(1, 65536, 32768) == 0


def _struct(n_rows=1, H=4, W=4, min_weight=0.5, min_depth=0.01, channels=3, H_dst=5, W_dst=6, eps=1e-3, occlusion=0.05, addr=None):
    pins = ((C.c_double * 4) * _lib.MAX_POSE_ROWS)()
    for i in range(_lib.MAX_POSE_ROWS):
        pins[i][:] = (4.0, 4.0, 1.5, 1.5)
    tab = (_lib.c_fp * _lib.MAX_POSE_ROWS)(*([addr] * _lib.MAX_POSE_ROWS))
    return _lib.BagsWarp(H, W, n_rows, min_weight, min_depth, channels, H_dst, W_dst, 0, eps, occlusion, pins, pins, tab, tab, tab, tab, tab, tab, tab,
                         tab, tab)


def test_entry_points_reject_bad_arguments_without_touching_the_gpu(lib):
    buf = (C.c_char * 65536)()
    addr = C.addressof(buf) + (-C.addressof(buf)) % 16
    err = lambda: lib.bags_last_error().decode()                                         # noqa: E731
    fwd = lambda a, ws=addr, n=1 << 20, loss=addr, stats=addr: lib.bags_warp_forward(C.byref(a), ws, n, loss, addr, stats, None)  # noqa: E731
    assert lib.bags_warp_forward(None, addr, 1 << 20, addr, addr, addr, None) == -1 and "null struct" in err()
    nan = float("nan")
    for kw, text in ((dict(n_rows=0), "n_rows"), (dict(n_rows=17), "n_rows"), (dict(H=0), "empty image"), (dict(H=65536, W=32768), "2^31"),
                     (dict(H_dst=0), "empty target"), (dict(W_dst=-1), "empty target"), (dict(H_dst=65536, W_dst=32768), "target image"),
                     (dict(channels=2), "must be 1 or 3"), (dict(channels=0), "must be 1 or 3"), (dict(channels=4), "must be 1 or 3"),
                     (dict(min_weight=0.0), "min_weight"), (dict(min_weight=nan), "min_weight"), (dict(min_depth=0.0), "min_depth"),
                     (dict(min_depth=math.inf), "min_depth"), (dict(eps=0.0), "eps"), (dict(eps=nan), "eps"), (dict(eps=math.inf), "eps"),
                     (dict(occlusion=0.0), "occlusion"), (dict(occlusion=-1.0), "occlusion"), (dict(occlusion=math.inf), "occlusion")):
        assert fwd(_struct(addr=addr, **kw)) == -1 and text in err(), (kw, err())
    a = _struct(addr=addr)
    a.pinhole_dst[0][1] = 0.0
    assert fwd(a) == -1 and "focal" in err()
    for field in ("depth", "weights", "view_src", "view_dst", "color_src", "image_dst"):
        a = _struct(addr=addr)
        getattr(a, field)[0] = None
        assert fwd(a) == -1 and "null " + field.replace("view_dst", "view_src") in err(), (field, err())
    for field in ("depth_dst", "weights_dst"):                # both or neither
        a = _struct(addr=addr)
        getattr(a, field)[0] = None
        assert fwd(a) == -1 and "together or not at all" in err(), (field, err())
    a = _struct(addr=addr, n_rows=2)
    a.depth_dst[1] = None
    assert fwd(a) == -1 and "depth_dst[1]" in err()
    a = _struct(addr=addr)
    assert fwd(a, loss=None) == -1 and "null loss" in err()
    assert fwd(a, ws=None) == -1 and "workspace" in err()
    assert fwd(a, n=8) == -1 and "needs a workspace of" in err()
    assert fwd(a, ws=addr + 8) == -1 and "16-byte aligned" in err()
    assert fwd(a, stats=addr + 4) == -1 and "8-byte aligned" in err()
    tab = (_lib.c_fp * 16)(*([addr] * 16))
    none = (_lib.c_fp * 16)()
    bwd = lambda stats=addr, g=addr, ws=addr, n=1 << 20, views=tab: lib.bags_warp_backward(C.byref(a), stats, g, ws, n, tab, tab, views, views, None)  # noqa: E731
    assert bwd(stats=None) == -1 and "null stats" in err()
    assert bwd(stats=addr + 4) == -1 and "8-byte aligned" in err()
    assert bwd(g=None) == -1 and "null g_loss" in err()
    assert bwd(ws=None) == -1 and "workspace" in err()                                    # a matrix gradient needs the workspace
    assert bwd(ws=addr + 8) == -1 and "16-byte aligned" in err()
    assert lib.bags_warp_backward(C.byref(a), addr, addr, None, 0, none, None, None, none, None) == 0         # nothing wanted
    assert lib.bags_warp_backward(C.byref(_struct(addr=addr, eps=0.0)), addr, addr, None, 0, none, None, None, none, None) == -1 and "eps" in err()
    a2 = _struct(addr=addr, n_rows=2)
    assert lib.bags_warp_image(C.byref(a2), addr, addr, None) == -1 and "one pair" in err()
    assert lib.bags_warp_image(None, addr, addr, None) == -1 and "null struct" in err()
    assert lib.bags_warp_image(C.byref(a), None, addr, None) == -1 and "null out" in err()
    assert lib.bags_warp_image(C.byref(a), addr, None, None) == -1 and "null out" in err()
    assert lib.bags_warp_image(C.byref(_struct(addr=addr, channels=2)), addr, addr, None) == -1 and "must be 1 or 3" in err()
    a.color_src[0] = None                                    # warp_image does not read the colours ...
    a.image_dst[0] = None                                    # ... but it samples the image
    assert lib.bags_warp_image(C.byref(a), addr, addr, None) == -1 and "null image_dst" in err()


def test_python_argument_errors():
    c = P.make_case(3, 5, 2, 3, 1e-3)
    D, A, Vi, Vj, col, img, cf, Dt, At = ([t[i] for i in range(2)] for t in (c["D"], c["A"], c["Vi"], c["Vj"], c["color"], c["image"], c["conf"],
                                                                              c["D_dst"], c["A_dst"]))
    pi, pj = c["pin_i"], c["pin_j"]
    for fn in (warp_loss, warp_loss_torch):
        with pytest.raises(ValueError, match="2 depth maps but 1 weights"):
            fn(D, A[:1], Vi, Vj, col, img, pi, pj)
        with pytest.raises(ValueError, match="2 depth maps but 1 view_dst"):
            fn(D, A, Vi, Vj[:1], col, img, pi, pj)
        with pytest.raises(ValueError, match=r"view_src\[1\] must be a \(4,4\)"):
            fn(D, A, [Vi[0], Vi[1][:3]], Vj, col, img, pi, pj)
        with pytest.raises(ValueError, match="2 depth maps but 1 color_src"):
            fn(D, A, Vi, Vj, col[:1], img, pi, pj)
        with pytest.raises(ValueError, match=r"color_src\[0\] has 2 channels, must be 1 or 3"):
            fn(D, A, Vi, Vj, [col[0][:2], col[1]], img, pi, pj)
        with pytest.raises(ValueError, match=r"color_src\[1\] is \(3, 3, 4\), expected \(C,3,5\)"):
            fn(D, A, Vi, Vj, [col[0], col[1][:, :, :4]], img, pi, pj)
        with pytest.raises(ValueError, match=r"image_dst\[0\] has 1 channels, expected 3"):
            fn(D, A, Vi, Vj, col, [img[0][:1], img[1]], pi, pj)
        with pytest.raises(ValueError, match=r"image_dst\[1\] is .* one size per call"):
            fn(D, A, Vi, Vj, col, [img[0], img[1][:, :4]], pi, pj)
        with pytest.raises(ValueError, match=r"image_dst\[0\] must be a non-empty \(C,H,W\)"):
            fn(D, A, Vi, Vj, col, [img[0][0], img[1]], pi, pj)
        with pytest.raises(ValueError, match="2 views but 3 pinholes"):
            fn(D, A, Vi, Vj, col, img, torch.cat([pi, pi[:1]]), pj)
        with pytest.raises(TypeError, match=r"\.float\(\)"):
            fn(D, A, Vi, Vj, col, img, pi, pj, [cf[0] > 0, cf[1]])
        with pytest.raises(ValueError, match="depth_dst and weights_dst must be given together"):
            fn(D, A, Vi, Vj, col, img, pi, pj, None, Dt)
        with pytest.raises(ValueError, match=r"depth_dst\[1\] and weights_dst\[1\] must be given together"):
            fn(D, A, Vi, Vj, col, img, pi, pj, None, [Dt[0], None], At)
        with pytest.raises(ValueError, match="2 depth maps but 1 weights_dst"):
            fn(D, A, Vi, Vj, col, img, pi, pj, None, Dt, At[:1])
        with pytest.raises(ValueError, match=r"depth_dst\[0\] is .* the target maps have the target image's size"):
            fn(D, A, Vi, Vj, col, img, pi, pj, None, [D[0], Dt[1]], At)
        for kw in (dict(min_weight=0.0), dict(min_depth=-1.0), dict(min_depth=math.inf), dict(eps=0.0), dict(eps=math.inf), dict(eps=float("nan")),
                   dict(occlusion=0.0), dict(occlusion=math.inf)):
            with pytest.raises(ValueError, match="must be a positive number"):
                fn(D, A, Vi, Vj, col, img, pi, pj, **kw)
    with pytest.raises(RuntimeError, match="AMD GPU"):       # a host map into the HIP path: refused, not copied
        warp_loss(D, A, Vi, Vj, col, img, pi, pj)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        warp_image(D[0], A[0], Vi[0], Vj[0], img[0], pi[0], pj[0])
    for fn in (warp_image, warp_image_torch):
        with pytest.raises(ValueError, match="one pair per call"):
            fn(D, A, Vi, Vj, img, pi, pj)
        with pytest.raises(ValueError, match="must be 1 or 3"):
            fn(D[0], A[0], Vi[0], Vj[0], img[0][:2], pi[0], pj[0])
        with pytest.raises(ValueError, match="occlusion must be a positive number"):
            fn(D[0], A[0], Vi[0], Vj[0], img[0], pi[0], pj[0], occlusion=0.0)
    loss, count = warp_loss_torch(D[0], A[0], Vi[0], Vj[0], col[0], img[0], pi[0], pj[0])            # one pair, no conf, no target maps
    assert tuple(loss.shape) == (1,) == tuple(count.shape) and count.item() == 15
    one = warp_loss_torch(D[0], A[0], Vi[0], Vj[0], col[0][:1], img[0][:1], pi[0], pj[0], None, [None], [None])[1]       # None entries: no test
    assert one.item() == 15
