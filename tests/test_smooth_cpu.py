"""CPU checks of bags_raster.depth_smooth_loss / normal_smooth_loss: the PyTorch statements against the published forms written out
literally (Monodepth2's get_smooth_loss, DN-Splatter's EdgeAwareTV and TVLoss) in float64; gradcheck; degenerate sizes and the empty
case; the argument errors of the Python names; the C entries' validation through the library, without a GPU; and the margin
condition that lets the GPU tests run the l1 penalty with eps = 0."""
import ctypes as C
import os
import re

import pytest
import torch

import smooth_cases as M
from bags_raster import _lib, depth_smooth_loss, depth_smooth_loss_torch, normal_smooth_loss, normal_smooth_loss_torch

F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------ published forms
def get_smooth_loss(disp, img):
    """Monodepth2, layers.py (disp (B,1,H,W), img (B,3,H,W))."""
    grad_disp_x = torch.abs(disp[:, :, :, :-1] - disp[:, :, :, 1:])
    grad_disp_y = torch.abs(disp[:, :, :-1, :] - disp[:, :, 1:, :])
    grad_img_x = torch.mean(torch.abs(img[:, :, :, :-1] - img[:, :, :, 1:]), 1, keepdim=True)
    grad_img_y = torch.mean(torch.abs(img[:, :, :-1, :] - img[:, :, 1:, :]), 1, keepdim=True)
    grad_disp_x = grad_disp_x * torch.exp(-grad_img_x)
    grad_disp_y = grad_disp_y * torch.exp(-grad_img_y)
    return grad_disp_x.mean() + grad_disp_y.mean()


def tv_loss(pred, square):
    """DN-Splatter's TVLoss on (3,H,W): the mean of the differences' penalty along each direction, added."""
    h_diff = pred[..., :, :-1] - pred[..., :, 1:]
    w_diff = pred[..., :-1, :] - pred[..., 1:, :]
    f = (lambda t: t * t) if square else torch.abs
    return torch.mean(f(h_diff)) + torch.mean(f(w_diff))


@pytest.mark.parametrize("H,W", ((5, 7), (33, 70)))
def test_the_statements_are_the_published_forms(H, W):
    """With everything valid (A = 1, no mask): Monodepth2's get_smooth_loss on the mean-normalised disparity (its trainer's
    `disp / (mean_disp + 1e-7)` without the 1e-7), DN-Splatter's EdgeAwareTV (the same lines on the depth as it is) and its TVLoss."""
    c = M.case("generic", H, W, 5)
    D = [t.double() for t in c["depth"]]
    one = [torch.ones_like(t) for t in D]
    rgb = [t.double() for t in c["rgb"]]
    N = [t.double() for t in c["normal"]]
    mono, _ = depth_smooth_loss_torch(D, one, rgb, space="inverse", normalize=True, order=1, penalty="l1", gamma=1.0)
    edge, cnt = depth_smooth_loss_torch(D, one, rgb, space="depth", normalize=False)
    tv2, _ = normal_smooth_loss_torch(N, one, None, penalty="l2")
    tv1, _ = normal_smooth_loss_torch(N, one, None, penalty="l1")
    assert mono.dtype == F64 and mono.shape == (5,)
    for v in range(5):
        disp = 1.0 / D[v][None]
        norm_disp = disp / disp.mean(2, True).mean(3, True)
        assert abs(mono[v].item() - get_smooth_loss(norm_disp, rgb[v][None]).item()) <= 1e-12
        assert abs(edge[v].item() - get_smooth_loss(D[v][None], rgb[v][None]).item()) <= 1e-12
        unit = N[v] / N[v].norm(dim=0, keepdim=True)
        assert abs(tv2[v].item() - tv_loss(unit, True).item()) <= 1e-12
        assert abs(tv1[v].item() - tv_loss(unit, False).item()) <= 1e-12
        assert cnt[v].item() == H * (W - 1) + (H - 1) * W


def test_the_second_order_is_zero_on_a_plane_in_inverse_depth():
    for (H, W) in ((5, 7), (33, 70)):
        cfg = M.config(order=2, eps=1e-3)
        l, n, gD, gA = M.forward_backward(depth_smooth_loss_torch, "plane", H, W, 5, cfg, False, F64, "cpu")
        assert (n > 0).all() and (l.abs() <= 1e-9).all() and all(torch.isfinite(g).all() for g in gD + gA)
        l1, _, _, _ = M.forward_backward(depth_smooth_loss_torch, "plane", H, W, 5, M.config(order=1, eps=1e-3), False, F64, "cpu")
        assert (l1 > 1e-3).all()                              # the first order is not


# ------------------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("order", (1, 2))
@pytest.mark.parametrize("penalty,eps", (("l2", 0.0), ("l1", 1e-2)))
def test_gradcheck(order, penalty, eps):
    """Also covers the closed-form -T / (mu n) term of the HIP backward's derivation: autograd through mu."""
    c = M.case("generic", 5, 7, 5)
    A = torch.stack(c["weights"][:2]).double().requires_grad_()
    D = torch.stack(c["depth"][:2]).double().requires_grad_()
    N = torch.stack(c["normal"][:2]).double().requires_grad_()
    rgb, m = [t.double() for t in c["rgb"][:2]], [t.double() for t in c["mask"][:2]]
    kw = dict(order=order, penalty=penalty, eps=eps, gamma=1.5)
    for normalize in (False, True):
        for space in ("inverse", "depth"):
            assert torch.autograd.gradcheck(lambda D, A: depth_smooth_loss_torch(list(D), list(A), rgb, m, space=space, normalize=normalize, **kw)[0],
                                            (D, A))
    assert torch.autograd.gradcheck(lambda N: normal_smooth_loss_torch(list(N), list(A.detach()), rgb, m, **kw)[0], (N,))
    assert torch.autograd.gradcheck(lambda N: normal_smooth_loss_torch(list(N), list(A.detach()), None, None, **kw)[0], (N,))


def test_holes_get_exact_zero_gradients():
    H, W = 33, 70
    kind = M.hole_kind(H, W)
    for normals, fn in ((False, depth_smooth_loss_torch), (True, normal_smooth_loss_torch)):
        dead = torch.zeros(H, W, dtype=torch.bool)
        for k in M.unusable_kinds(normals):
            dead |= kind == k
        for cfg in (M.HOLES_CONFIGS if not normals else M.HOLES_CONFIGS[:2]):
            l, n, gF, gA = M.forward_backward(fn, "holes", H, W, 5, cfg, normals, F64, "cpu")
            assert torch.isfinite(l).all() and (n > 0).all()
            for v in range(5):
                assert torch.isfinite(gF[v]).all() and torch.isfinite(gA[v]).all()
                assert (gF[v][:, dead] == 0).all() and (gA[v][:, dead] == 0).all() and gF[v][:, kind > 4].abs().max() > 0
                if cfg["masked"]:
                    assert (gF[v][:, M.case("holes", H, W, 5)["mask"][v] == 0] == 0).all()


def test_degenerate_sizes_and_the_empty_case_are_exact_zeros():
    for normals, fn in ((False, depth_smooth_loss_torch), (True, normal_smooth_loss_torch)):
        for order in (1, 2):
            for cfg in (M.config(order=order), M.config(order=order, penalty="l2", normalize=False, guide="none", masked=False)):
                for (H, W) in M.SIZES:
                    l, n, gF, gA = M.forward_backward(fn, "empty", H, W, 5, cfg, normals, F64, "cpu")
                    assert (l == 0).all() and (n == 0).all() and all((g == 0).all() for g in gF + gA)
                for (H, W) in ((1, 1), (2, 2))[:order]:        # too small for the order: no stencil
                    l, n, gF, gA = M.forward_backward(fn, "generic", H, W, 5, cfg, normals, F64, "cpu")
                    assert (l == 0).all() and (n == 0).all() and all((g == 0).all() for g in gF + gA)
                l, n, _, _ = M.forward_backward(fn, "generic", 1, 5, 5, dict(cfg, masked=False), normals, F64, "cpu")
                assert (n == (4 if order == 1 else 3)).all() and (l > 0).all()      # one row: the horizontal stencils alone
                l32, n32, _, _ = M.forward_backward(fn, "generic", 5, 7, 5, cfg, normals, F32, "cpu")
                l64, n64, _, _ = M.forward_backward(fn, "generic", 5, 7, 5, cfg, normals, F64, "cpu")
                assert l32.dtype == F32 and ((l32.double() - l64).abs() <= 1e-5 * (1 + l64.abs())).all()


# ------------------------------------------------------------------------------------------------------------ the margin condition
def test_the_margin_condition_holds_wherever_the_gpu_tests_run_l1_with_eps_0():
    """The depth field comes from one float32 division, so against the float64 reference d is off by up to 4 * 2^-24 * max|x| at
    order 2; a run with the l1 penalty and eps = 0 must have every |d| >= 8 * 2^-24 * max|x| in the float64 reference, or a sign --
    a whole unit of the gradient -- could legitimately differ.  (The normals field is formed in float64 on both sides.)"""
    runs = set()
    for (H, W) in M.SIZES:
        for V in M.VIEWS:
            for cfg in M.depth_configs(M.eps_l1_of(H, W, V)):
                if cfg["penalty"] == "l1" and cfg["eps"] == 0:
                    runs.add(("generic", H, W, V, cfg["order"], cfg["space"]))
    for (H, W, V) in M.HOLES_SIZES:
        for cfg in M.HOLES_CONFIGS:
            if cfg["penalty"] == "l1" and cfg["eps"] == 0:
                runs.add(("holes", H, W, V, cfg["order"], cfg["space"]))
    assert len(runs) > 50                                      # (the bit-for-bit tests compare HIP with HIP: no margin needed)
    for (name, H, W, V, order, space) in sorted(runs):
        small, big = M.smallest_difference(name, H, W, V, order, space)
        assert small >= M.MARGIN * big, (name, H, W, V, order, space, small, M.MARGIN * big)
    assert M.eps_l1_of(64, 256, 17) == 1e-3 and M.eps_l1_of(64, 256, 1) == 0.0


# ------------------------------------------------------------------------------------------------------------ arguments
def test_argument_errors():
    c = M.case("generic", 5, 7, 5)
    D, N, A, rgb, m = c["depth"], c["normal"], c["weights"], c["rgb"], c["mask"]
    for fn, F in ((depth_smooth_loss_torch, D), (depth_smooth_loss, D), (normal_smooth_loss_torch, N), (normal_smooth_loss, N)):
        with pytest.raises(TypeError, match="bool"):
            fn(F[0], A[0], rgb[0], m[0] > 0)
        with pytest.raises(ValueError):
            fn(F[0][:, :3], A[0])                             # another size than the weights
        with pytest.raises(ValueError):
            fn(F[0], A[0][:, :3])
        with pytest.raises(ValueError):
            fn(F[0], A[0], rgb[0][:2])                        # a guide of two channels
        with pytest.raises(ValueError):
            fn(F[0], A[0], rgb[0][:, :3])
        with pytest.raises(ValueError):
            fn(F[:2], A[:2], [rgb[0], None])                  # guide=None is for the whole call
        with pytest.raises(ValueError):
            fn(F[:2], A[:2], [rgb[0], c["gray"][1]])          # one channel count per call
        with pytest.raises(ValueError):
            fn(F[:2], A[:3])
        with pytest.raises(ValueError):
            fn(F[:2], A[:2], rgb[:3])
        with pytest.raises(ValueError):
            fn(F[:2], A[:2], rgb[:2], m[:3])
        for order in (0, 3, 1.5, "1"):
            with pytest.raises(ValueError, match="order"):
                fn(F[0], A[0], order=order)
        with pytest.raises(ValueError, match="penalty"):
            fn(F[0], A[0], penalty="huber")
        with pytest.raises(ValueError, match="eps"):
            fn(F[0], A[0], penalty="l2", eps=1e-3)
        with pytest.raises(ValueError, match="eps"):
            fn(F[0], A[0], eps=-1e-3)
        with pytest.raises(ValueError, match="gamma"):
            fn(F[0], A[0], gamma=-1.0)
        with pytest.raises(ValueError, match="gamma"):
            fn(F[0], A[0], gamma=float("nan"))
    for fn in (depth_smooth_loss_torch, depth_smooth_loss):
        with pytest.raises(ValueError, match="space"):
            fn(D[0], A[0], space="disparity")
        with pytest.raises(ValueError):
            fn(N[0], A[0])                                    # not (H,W) or (1,H,W)
    for fn in (normal_smooth_loss_torch, normal_smooth_loss):
        with pytest.raises(ValueError):
            fn(D[0], A[0])                                    # not (3,H,W)
        with pytest.raises(ValueError, match="min_norm"):
            fn(N[0], A[0], min_norm=-1.0)
    with pytest.raises(RuntimeError, match="AMD GPU.*depth_smooth_loss_torch"):
        depth_smooth_loss(D[0], A[0], rgb[0], m[0])           # no CPU fallback behind the HIP names
    with pytest.raises(RuntimeError, match="AMD GPU.*normal_smooth_loss_torch"):
        normal_smooth_loss(N[0], A[0])


def test_the_header_and_the_ctypes_side_agree(lib):
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    assert re.search(r"#define BAGS_ABI_VERSION 11\b", header) and _lib.ABI_VERSION == 11 and lib.bags_abi_version() == 11
    for name, value in (("TILE_W", _lib.SMOOTH_TILE_W), ("TILE_H", _lib.SMOOTH_TILE_H), ("PARTIALS", _lib.SMOOTH_PARTIALS),
                        ("STATS", _lib.SMOOTH_STATS), ("MEAN_SLOTS", _lib.SMOOTH_MEAN_SLOTS), ("DEPTH", _lib.SMOOTH_DEPTH),
                        ("NORMAL", _lib.SMOOTH_NORMAL), ("L1", _lib.SMOOTH_L1), ("L2", _lib.SMOOTH_L2)):
        assert re.search(r"#define BAGS_SMOOTH_%s %d\b" % (name, value), header), name
    body = re.search(r"typedef struct BagsSmooth \{(.*?)\} BagsSmooth;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|$)", decl.strip())]
    assert declared == [n for n, _ in _lib.BagsSmooth._fields_], declared
    assert C.sizeof(_lib.BagsSmooth) == 10 * 4 + 2 * 4 + 2 * 8 + 4 * 16 * 8
    for name in ("bags_smooth_workspace_size", "bags_smooth_forward", "bags_smooth_backward"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\((.*?)\);" % name, header, re.S).group(1)
        if name != "bags_smooth_workspace_size":
            assert decl.rstrip().endswith("void* stream") and _lib.SYMBOLS[name][1][-1] is C.c_void_p, name


def test_the_c_entries_validate_their_arguments(lib):
    """Reported before anything is enqueued: no GPU touched.  Host addresses stand in for device pointers."""
    buf = (C.c_double * 4096)()
    addr = (C.addressof(buf) + 15) & ~15                      # 16-byte aligned, as the workspace must be
    field = lambda n: (_lib.c_fp * _lib.MAX_POSE_ROWS)(*([addr] * n + [None] * (_lib.MAX_POSE_ROWS - n)))      # noqa: E731
    err = lambda: lib.bags_last_error()                                                                      # noqa: E731

    def make(kind=0, space=1, order=1, penalty=0, normalize=1, H=8, W=8, n=2, cg=3, mw=0.5, mn=0.1, eps=0.0, gamma=1.0, have=2, guides=2):
        return _lib.BagsSmooth(kind, space, order, penalty, normalize, H, W, n, cg, 0, mw, mn, eps, gamma, field(have), field(have), field(guides),
                               field(0))
    size = lib.bags_smooth_workspace_size
    assert size(0, 8, 8) == 0 and size(17, 8, 8) == 0 and size(1, 0, 8) == 0 and size(1, 65536, 65536) == 0
    tiles = ((1920 + 31) // 32) * ((1080 + 7) // 8)
    assert size(2, 8, 8) >= 2 * (6 + 2) * 8 and size(16, 1080, 1920) > size(1, 1080, 1920) >= (tiles * 6 + 512 * 2) * 8
    fwd = lambda a, ws=addr, nb=1 << 20, loss=addr, count=addr, stats=addr: lib.bags_smooth_forward(C.byref(a), ws, nb, loss, count, stats, None)     # noqa: E731
    assert lib.bags_smooth_forward(None, addr, 1 << 20, addr, addr, addr, None) == -1 and b"null struct" in err()
    assert fwd(make(kind=2)) == -1 and b"unknown kind" in err()
    assert fwd(make(space=2)) == -1 and b"unknown space" in err()
    for order in (0, 3):
        assert fwd(make(order=order)) == -1 and b"order" in err()
    assert fwd(make(penalty=2)) == -1 and b"unknown penalty" in err()
    assert fwd(make(normalize=2)) == -1 and b"normalize" in err()
    assert fwd(make(kind=1, normalize=1)) == -1 and b"normalize" in err()
    for n in (0, 17):
        assert fwd(make(n=n)) == -1 and b"n_rows" in err()
    assert fwd(make(H=0)) == -1 and b"empty image" in err()
    assert fwd(make(H=65536, W=65536)) == -1 and b"2^31" in err()
    assert fwd(make(cg=2)) == -1 and b"guide_channels" in err()
    assert fwd(make(mw=float("nan"))) == -1 and b"min_weight" in err()
    assert fwd(make(kind=1, normalize=0, mn=-0.1)) == -1 and b"min_norm" in err()
    assert fwd(make(eps=-1.0)) == -1 and b"eps" in err()
    assert fwd(make(penalty=1, eps=1e-3)) == -1 and b"eps must be 0" in err()
    assert fwd(make(gamma=-1.0)) == -1 and b"gamma" in err()
    assert fwd(make(gamma=float("inf"))) == -1 and b"gamma" in err()
    assert fwd(make(have=1)) == -1 and b"null field[1]" in err()           # fewer pointers than n_rows says
    assert fwd(make(guides=1)) == -1 and b"null guide[1]" in err()
    assert fwd(make(), loss=None) == -1 and b"null loss" in err()
    assert fwd(make(), ws=None) == -1 and b"workspace" in err()
    assert fwd(make(), nb=8) == -1 and b"workspace" in err()
    assert fwd(make(), ws=addr + 8) == -1 and b"16-byte" in err()
    assert fwd(make(), stats=addr + 4) == -1 and b"8-byte" in err()
    bwd = lambda a, stats=addr, g=addr, gf=field(2), gw=field(2): lib.bags_smooth_backward(C.byref(a), stats, g, gf, gw, None)      # noqa: E731
    assert bwd(make(), stats=None) == -1 and b"null stats" in err()
    assert bwd(make(), g=None) == -1 and b"null g_loss" in err()
    assert bwd(make(order=7)) == -1 and b"order" in err()
    assert bwd(make(), gf=field(0), gw=field(0)) == 0 and bwd(make(), gf=None, gw=None) == 0      # nothing wanted: a successful no-op
    assert bwd(make(kind=1, normalize=0), gf=field(0), gw=field(2)) == 0                          # the normal kind has no weights gradient
