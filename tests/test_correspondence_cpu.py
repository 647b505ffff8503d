"""No-GPU checks of the correspondence loss (bags_raster/correspondence.py, csrc/correspondence.hip): gradcheck of the PyTorch
statement, the statement against the closed forms, that the bars of tests/correspondence_cases.py reject wrong answers, the
generator's conditions, the degenerate pairs in float64, reproject_pixels_torch on a fronto-parallel plane, the C surface and the
rejections of its entry points and of the Python wrappers."""
import ctypes as C
import math
import os

import pytest
import torch

import correspondence_cases as P
import bags_raster
from bags_raster import _lib, correspondence_loss, correspondence_loss_torch, reproject_pixels, reproject_pixels_torch

FUNCS = ("bags_correspondence_workspace_size", "bags_correspondence_forward", "bags_correspondence_backward", "bags_reproject_pixels")
PUBLIC = ("correspondence_loss", "correspondence_loss_torch", "reproject_pixels", "reproject_pixels_torch")
F64 = torch.float64
IDS = ["%dx%d" % s for s in P.SHAPES]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ---------------------------------------------------------------------------------------------------------------- the function
def _round_off(a, b, s):
    """|a - b| within float64 round-off of the sum of the absolute values of the terms ``s``, element by element; exact where ``s`` is 0.
    The residual r = proj - match is itself a difference of two numbers of some tens of pixels, which ``s`` does not see: where the
    match noise is nearly zero the gradient carries that cancellation, hence the second term, from the largest element."""
    return bool(((a - b).abs() <= torch.where(s > 0, 1e-11 * s + 1e-13 * s.max(), torch.zeros_like(s))).all())


@pytest.mark.parametrize("delta", P.DELTAS)
def test_gradcheck_of_the_statement(delta):
    c = P.make_case(3, 5, 2, delta)
    leaf = lambda t: t.double().clone().requires_grad_(True)                             # noqa: E731
    D, A, Vi, Vj = leaf(c["D"][0]), leaf(c["A"][0]), leaf(c["Vi"][0]), leaf(c["Vj"][0])
    f = lambda D, A, Vi, Vj: correspondence_loss_torch(D, A, Vi, Vj, c["match"][0].double(), c["pin_i"][0], c["pin_j"][0], c["conf"][0].double(),  # noqa: E731
                                                       delta=delta, min_weight=P.MIN_WEIGHT, min_depth=P.MIN_DEPTH)[0]
    assert f(D, A, Vi, Vj).item() > 0
    assert torch.autograd.gradcheck(f, (D, A, Vi, Vj))


@pytest.mark.parametrize("delta", P.DELTAS)
@pytest.mark.parametrize("H,W", P.SHAPES, ids=IDS)
def test_statement_equals_the_closed_forms(H, W, delta):
    """correspondence_loss_torch in float64 with autograd against the closed forms of the loss and of the four gradients, element by
    element to round-off; exact zeros where the closed form has zeros (invalid pixels, the fourth columns)."""
    for K in (2, 17):
        c = P.make_case(H, W, K, delta)
        ref, want = P.reference(H, W, K, delta), P.closed_form(c)
        for name, a, b, s in zip(P.NAMES, ref[:5], want, P.scales(c)):
            assert a.shape == b.shape and torch.isfinite(a).all(), name
            assert _round_off(a, b, s), (name, float(((a - b).abs() / s.clamp_min(1e-300)).max()))
            assert bool(((b == 0) <= (a == 0)).all()), name
        assert (ref[5] - P._pieces(c)["cnt"]).abs().max() < 1e-12
        assert (ref[0] > 0).all() and (ref[5] > 0).all() and all(t.abs().max() > 0 for t in ref[1:5])
        assert ref[3][:, :, 3].abs().max() == 0 and ref[4][:, :, 3].abs().max() == 0


def test_bars_reject_wrong_answers():
    """The closed forms are far inside the bars on every case; each of the four wrong answers is outside a bar on at least one case
    (and where it is said below, on every case of at least 200 pixels)."""
    hit = dict(transpose=0, flip_dA=0, n_is_pixels=0, drop_delta_over_e=0)
    for H, W in P.SHAPES:
        for K in P.PAIRS:
            for delta in P.DELTAS:
                c = P.make_case(H, W, K, delta)
                good = P.margins(H, W, K, delta, P.closed_form(c))
                assert all(m <= 1e-3 for m in good), (H, W, K, delta, good)
                big = H * W >= 200
                m = P.margins(H, W, K, delta, P.closed_form(c, transpose=True))
                hit["transpose"] += max(m) > 1.0
                assert not big or (m[0] > 1.0 and m[3] > 1.0 and m[4] > 1.0), ("transpose", H, W, K, delta, m)
                m = P.margins(H, W, K, delta, P.closed_form(c, flip_dA=True))
                hit["flip_dA"] += m[2] > 1.0
                assert m[0] <= 1e-3 and m[1] <= 1e-3 and m[2] > 1.0 and m[3] <= 1e-3, ("flip_dA", H, W, K, delta, m)
                m = P.margins(H, W, K, delta, P.closed_form(c, n_is_pixels=True))
                hit["n_is_pixels"] += max(m[1:]) > 1.0
                assert m[0] <= 1e-3 and all(x > 1.0 for x in m[1:]), ("n_is_pixels", H, W, K, delta, m)
                if math.isfinite(delta):
                    m = P.margins(H, W, K, delta, P.closed_form(c, drop_delta_over_e=True))
                    hit["drop_delta_over_e"] += max(m[1:]) > 1.0
                    assert not big or all(x > 1.0 for x in m[1:]), ("drop_delta_over_e", H, W, K, delta, m)
    assert all(v > 0 for v in hit.values()), hit


def test_generator_conditions_hold_on_every_case():
    worst = dict(gap=1.0, front=1.0, valid=1.0)
    linear = []
    for H, W in P.SHAPES:
        for K in P.PAIRS:
            for delta in P.DELTAS:
                f = P.check_case(P.make_case(H, W, K, delta))
                for k in worst:
                    worst[k] = min(worst[k], f[k])
                if f["linear"] is not None:
                    linear.append(f["linear"])
    for delta in P.DELTAS:
        P.check_case(P.degenerate_case(delta))
    print("\ncorrespondence cases: smallest |A - min_weight| %.3g, |x_j.z - min_depth| %.3g, valid share %.3f; linear share %.2f .. %.2f"
          % (worst["gap"], worst["front"], worst["valid"], min(linear), max(linear)))
    assert worst["valid"] >= 0.5 and linear
    assert P.SEAM[0] * P.SEAM[1] > 2 * P.CHUNK and (P.SEAM[0] * P.SEAM[1]) % P.CHUNK != 0
    assert P.make_case(17, 67, 2, 1.0) is P.make_case(17, 67, 2, 1.0)                     # cached, shared
    pins = P.make_case(17, 67, 2, 1.0)
    assert (pins["pin_i"] - pins["pin_j"]).abs().min() > 0                                 # different pinholes on the two sides


@pytest.mark.parametrize("delta", P.DELTAS)
def test_degenerate_pairs_give_zero_loss_and_zero_gradients(delta):
    c = P.degenerate_case(delta)
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


def test_a_global_alignment_with_a_scale_leaves_the_loss_unchanged():
    """x_cam = X_w @ A + b: replacing both matrices by G @ V for one invertible G (a similarity with a shear) changes neither M nor
    c -- the reason the statement takes the true inverse."""
    c = P.make_case(17, 67, 2, 1.0)
    G = torch.eye(4, dtype=F64)
    G[:3, :3] = 0.7 * P.so3_exp(torch.tensor((0.2, -0.4, 0.1))).double()
    G[0, 2] += 0.1
    G[3, :3] = torch.tensor((0.3, -0.2, 0.5), dtype=F64)
    run = lambda Vi, Vj: correspondence_loss_torch(c["D"][0].double(), c["A"][0].double(), Vi, Vj, c["match"][0].double(), c["pin_i"][0],  # noqa: E731
                                                   c["pin_j"][0], c["conf"][0].double())
    a, b = run(c["Vi"][0].double(), c["Vj"][0].double()), run(G @ c["Vi"][0].double(), G @ c["Vj"][0].double())
    assert a[0].item() > 0 and abs(a[0].item() - b[0].item()) <= 1e-11 * a[0].item() and a[1].item() == b[1].item()


def test_reproject_pixels_torch_on_a_fronto_parallel_plane():
    """A wall at depth z0 seen by two axis-aligned cameras a baseline t apart: proj = (fx_j (x_i.x + t_x) / z0 + cx_j, ...) in closed
    form, and valid exactly where that lies inside the target image."""
    H, W, z0 = 9, 14, 2.5
    pi, pj = (12.0, 11.0, 6.25, 4.5), (10.0, 10.5, 5.75, 3.25)
    A = torch.full((1, H, W), 0.8125, dtype=F64)
    D = A * z0
    A[0, 2, 3] = 0.25                                        # a hole
    Vi, Vj = torch.eye(4, dtype=F64), torch.eye(4, dtype=F64)
    Vj[3, :3] = torch.tensor((0.4, -0.3, 0.0), dtype=F64)
    proj, valid = reproject_pixels_torch(D, A, Vi, Vj, pi, pj, (7, 11))
    assert proj.dtype == F64 and tuple(proj.shape) == (2, H, W) and valid.dtype == torch.bool and tuple(valid.shape) == (H, W)
    u = torch.arange(W, dtype=F64)[None, :].expand(H, W)
    v = torch.arange(H, dtype=F64)[:, None].expand(H, W)
    x = pj[0] * (z0 * (u - pi[2]) / pi[0] + 0.4) / z0 + pj[2]
    y = pj[1] * (z0 * (v - pi[3]) / pi[1] - 0.3) / z0 + pj[3]
    hole = torch.zeros(H, W, dtype=torch.bool)
    hole[2, 3] = True
    want = torch.where(hole, torch.zeros_like(x), x), torch.where(hole, torch.zeros_like(y), y)
    assert (proj[0] - want[0]).abs().max() <= 1e-12 and (proj[1] - want[1]).abs().max() <= 1e-12
    inside = (x >= -0.5) & (x < 11 - 0.5) & (y >= -0.5) & (y < 7 - 0.5) & ~hole
    assert torch.equal(valid, inside) and inside.any() and (~inside).any()
    # the matches reproject_pixels_torch gives have zero loss
    loss, count = correspondence_loss_torch(D, A, Vi, Vj, proj, pi, pj)
    assert loss.item() <= 1e-24 and count.item() == H * W - 1
    # a target behind the camera: nothing projects
    Vj[3, 2] = -5.0
    proj, valid = reproject_pixels_torch(D, A, Vi, Vj, pi, pj, (7, 11))
    assert not valid.any() and proj.abs().max() == 0


# ---------------------------------------------------------------------------------------------------------------- the surface
def test_public_names_and_c_surface(lib):
    for name in PUBLIC:
        assert getattr(bags_raster, name) is not None and name in bags_raster.__all__, name
    for name in FUNCS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 11 and lib.bags_abi_version() == 11
    assert _lib.CORRESPONDENCE_CHUNK == 256 and _lib.CORRESPONDENCE_STATS == 2 and _lib.CORRESPONDENCE_SUMS == 12
    assert C.sizeof(_lib.BagsCorrespondence) == 16 + 2 * 8 + 2 * 16 * 4 * 8 + 6 * 16 * 8
    size = lib.bags_correspondence_workspace_size
    chunks = lambda H, W: -(-H * W // 256)                                               # noqa: E731
    assert 12 * 8 <= size(1, 1, 1) <= 256 and size(16, 1080, 1920) == 16 * chunks(1080, 1920) * 12 * 8 and 3 * 3 * 12 * 8 <= size(3, 7, 92) <= 1024
    assert size(0, 4, 4) == 0 and size(17, 4, 4) == 0 and size(1, 0, 4) == 0 and size(1, 65536, 32768) == 0


def _struct(n_rows=1, H=4, W=4, min_weight=0.5, min_depth=0.01, delta=1.0, addr=None):
    pins = ((C.c_double * 4) * _lib.MAX_POSE_ROWS)()
    for i in range(_lib.MAX_POSE_ROWS):
        pins[i][:] = (4.0, 4.0, 1.5, 1.5)
    tab = (_lib.c_fp * _lib.MAX_POSE_ROWS)(*([addr] * _lib.MAX_POSE_ROWS))
    return _lib.BagsCorrespondence(H, W, n_rows, min_weight, min_depth, delta, pins, pins, tab, tab, tab, tab, tab, tab)


def test_entry_points_reject_bad_arguments_without_touching_the_gpu(lib):
    buf = (C.c_char * 65536)()
    addr = C.addressof(buf) + (-C.addressof(buf)) % 16
    err = lambda: lib.bags_last_error().decode()                                         # noqa: E731
    fwd = lambda a, ws=addr, n=1 << 20, loss=addr, stats=addr: lib.bags_correspondence_forward(C.byref(a), ws, n, loss, addr, stats, None)  # noqa: E731
    assert lib.bags_correspondence_forward(None, addr, 1 << 20, addr, addr, addr, None) == -1 and "null struct" in err()
    for kw, text in ((dict(n_rows=0), "n_rows"), (dict(n_rows=17), "n_rows"), (dict(H=0), "empty image"), (dict(H=65536, W=32768), "2^31"),
                     (dict(min_weight=0.0), "min_weight"), (dict(min_weight=float("nan")), "min_weight"), (dict(min_depth=0.0), "min_depth"),
                     (dict(min_depth=math.inf), "min_depth"), (dict(delta=0.0), "delta"), (dict(delta=float("nan")), "delta")):
        assert fwd(_struct(addr=addr, **kw)) == -1 and text in err(), (kw, err())
    a = _struct(addr=addr)
    a.pinhole_dst[0][1] = 0.0
    assert fwd(a) == -1 and "focal" in err()
    for field in ("depth", "weights", "match", "view_src", "view_dst"):
        a = _struct(addr=addr)
        getattr(a, field)[0] = None
        assert fwd(a) == -1 and "null " + field.replace("view_dst", "view_src") in err(), (field, err())
    a = _struct(addr=addr)
    assert fwd(a, loss=None) == -1 and "null loss" in err()
    assert fwd(a, ws=None) == -1 and "workspace" in err()
    assert fwd(a, n=8) == -1 and "needs a workspace of" in err()
    assert fwd(a, ws=addr + 8) == -1 and "16-byte aligned" in err()
    assert fwd(a, stats=addr + 4) == -1 and "8-byte aligned" in err()
    tab = (_lib.c_fp * 16)(*([addr] * 16))
    none = (_lib.c_fp * 16)()
    bwd = lambda stats=addr, g=addr, ws=addr, n=1 << 20, views=tab: lib.bags_correspondence_backward(C.byref(a), stats, g, ws, n, tab, tab, views,  # noqa: E731
                                                                                                     views, None)
    assert bwd(stats=None) == -1 and "null stats" in err()
    assert bwd(g=None) == -1 and "null g_loss" in err()
    assert bwd(ws=None) == -1 and "workspace" in err()                                    # a matrix gradient needs the workspace
    assert lib.bags_correspondence_backward(C.byref(a), addr, addr, None, 0, none, None, None, none, None) == 0         # nothing wanted
    a2 = _struct(addr=addr, n_rows=2)
    assert lib.bags_reproject_pixels(C.byref(a2), 4, 4, addr, addr, None) == -1 and "one pair" in err()
    assert lib.bags_reproject_pixels(C.byref(a), 0, 4, addr, addr, None) == -1 and "empty target" in err()
    assert lib.bags_reproject_pixels(C.byref(a), 4, 4, None, addr, None) == -1 and "null proj" in err()
    a.match[0] = None                                        # reproject_pixels does not read the matches
    assert lib.bags_reproject_pixels(C.byref(a), 4, 0, addr, addr, None) == -1 and "empty target" in err()


def test_python_argument_errors():
    c = P.make_case(3, 5, 2, 1.0)
    D, A, Vi, Vj, m, cf = ([t[i] for i in range(2)] for t in (c["D"], c["A"], c["Vi"], c["Vj"], c["match"], c["conf"]))
    pi, pj = c["pin_i"], c["pin_j"]
    for fn in (correspondence_loss, correspondence_loss_torch):
        with pytest.raises(ValueError, match="2 depth maps but 1 weights"):
            fn(D, A[:1], Vi, Vj, m, pi, pj)
        with pytest.raises(ValueError, match="2 depth maps but 1 view_dst"):
            fn(D, A, Vi, Vj[:1], m, pi, pj)
        with pytest.raises(ValueError, match=r"view_src\[1\] must be a \(4,4\)"):
            fn(D, A, [Vi[0], Vi[1][:3]], Vj, m, pi, pj)
        with pytest.raises(ValueError, match=r"match\[0\] must be \(2,H,W\)"):
            fn(D, A, Vi, Vj, [m[0][:1], m[1]], pi, pj)
        with pytest.raises(ValueError, match="2 views but 3 pinholes"):
            fn(D, A, Vi, Vj, m, torch.cat([pi, pi[:1]]), pj)
        with pytest.raises(TypeError, match=r"\.float\(\)"):
            fn(D, A, Vi, Vj, m, pi, pj, [cf[0] > 0, cf[1]])
        for kw in (dict(min_weight=0.0), dict(min_depth=-1.0), dict(min_depth=math.inf), dict(delta=0.0), dict(delta=float("nan"))):
            with pytest.raises(ValueError, match="must be a positive number"):
                fn(D, A, Vi, Vj, m, pi, pj, **kw)
    with pytest.raises(RuntimeError, match="AMD GPU"):       # a host map into the HIP path: refused, not copied
        correspondence_loss(D, A, Vi, Vj, m, pi, pj)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        reproject_pixels(D[0], A[0], Vi[0], Vj[0], pi[0], pj[0], (3, 5))
    for fn in (reproject_pixels, reproject_pixels_torch):
        with pytest.raises(ValueError, match="one pair per call"):
            fn(D, A, Vi, Vj, pi, pj, (3, 5))
        with pytest.raises(ValueError, match="size_dst"):
            fn(D[0], A[0], Vi[0], Vj[0], pi[0], pj[0], (0, 5))
    loss, count = correspondence_loss_torch(D[0], A[0], Vi[0], Vj[0], m[0], pi[0], pj[0], delta=math.inf)        # one pair, no conf
    assert tuple(loss.shape) == (1,) == tuple(count.shape) and count.item() == 15
