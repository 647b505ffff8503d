"""CPU checks of bags_raster.normal_map_loss: the PyTorch statement against independent float64 lines (F.normalize, torch.where) on
the case images of tests/normal_map_cases.py; gradcheck; the argument errors of the Python names; the C entries' validation
through the library, without a GPU."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import normal_map_cases as M
from bags_raster import _lib, normal_map_loss, normal_map_loss_torch

F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def independent(c, v, mode, masked):
    """(loss, count) of view v in float64, the ten lines a user writes today."""
    N, A, p = c["normal"][v].double(), c["weights"][v].double()[0], c["target"][v].double()
    m = c["mask"][v].double() if masked else torch.ones_like(A)
    nn, pp = (N * N).sum(0), (p * p).sum(0)
    valid = (A >= M.MIN_WEIGHT) & torch.isfinite(nn) & (nn > float(torch.tensor(M.MIN_NORM)) ** 2) & (m > 0) & torch.isfinite(pp) & (pp > 0.25)
    nh = F.normalize(torch.where(valid, N, torch.ones_like(N)), dim=0)
    ph = F.normalize(torch.where(valid, p, torch.ones_like(p)), dim=0)
    l = (nh - ph).abs().sum(0) if mode == "l1" else 1 - (nh * ph).sum(0)
    w = torch.where(valid, m, torch.zeros_like(m))
    cnt = w.sum()
    return ((w * l).sum() / cnt if cnt > 0 else torch.zeros((), dtype=F64)), cnt


@pytest.mark.parametrize("name", M.CASES)
@pytest.mark.parametrize("mode", ("cos", "l1"))
def test_the_statement_against_independent_lines(name, mode):
    for (H, W) in M.SIZES:
        for masked in (False, True):
            c = M.case(name, H, W, 5)
            l64, n64, g64 = M.forward_backward(normal_map_loss_torch, name, H, W, 5, mode, masked, F64, "cpu")
            l32, n32, g32 = M.forward_backward(normal_map_loss_torch, name, H, W, 5, mode, masked, F32, "cpu")
            assert l32.dtype == F32 and l64.dtype == F64 and l64.shape == (5,) and n64.shape == (5,)
            for v in range(5):
                ref_l, ref_n = independent(c, v, mode, masked)
                assert abs(l64[v].item() - ref_l.item()) <= 1e-12 and abs(n64[v].item() - ref_n.item()) <= 1e-9
                assert abs(l32[v].item() - ref_l.item()) <= 1e-5 * (1 + abs(ref_l.item()))
                assert torch.isfinite(g64[v]).all() and torch.isfinite(g32[v]).all()
            if name == "empty" or (name == "depth_target" and min(H, W) < 3):
                assert (l64 == 0).all() and (n64 == 0).all() and all((g == 0).all() for g in g64)
            elif H * W >= 100:                                # (a few pixels may all be holes, or all masked)
                assert (n64 > 0).all()


def test_holes_get_exact_zero_gradients():
    H, W = 33, 70
    kind = M.hole_kind(H, W)
    for mode in ("cos", "l1"):
        l, n, g = M.forward_backward(normal_map_loss_torch, "holes", H, W, 5, mode, True, F64, "cpu")
        assert torch.isfinite(l).all() and (n > 0).all()
        for v in range(5):
            assert (g[v][:, kind <= 4] == 0).all() and g[v][:, kind > 4].abs().max() > 0
            assert (g[v][:, M.case("holes", H, W, 5)["mask"][v] == 0] == 0).all()


def test_gradcheck():
    c = M.case("generic", 5, 7, 5)
    N = torch.stack(c["normal"][:2]).double().requires_grad_()
    A, p, m = [t.double() for t in c["weights"][:2]], [t.double() for t in c["target"][:2]], [t.double() for t in c["mask"][:2]]
    for mode in ("cos", "l1"):
        assert torch.autograd.gradcheck(lambda N: normal_map_loss_torch(list(N), A, p, m, mode=mode)[0], (N,))


def test_argument_errors():
    c = M.case("generic", 5, 7, 5)
    N, A, p, m = c["normal"], c["weights"], c["target"], c["mask"]
    for fn in (normal_map_loss_torch, normal_map_loss):
        with pytest.raises(ValueError):
            fn(N[0][:2], A[0], p[0])                          # not (3,H,W)
        with pytest.raises(ValueError):
            fn(N[0], A[0][:, :3], p[0])                       # another size
        with pytest.raises(ValueError):
            fn(N[0], A[0], p[0][:, :, :3])
        with pytest.raises(ValueError):
            fn(N[:2], A[:2], p[:3])                           # more targets than views
        with pytest.raises(ValueError):
            fn(N[:2], A[:3], p[:2])
        with pytest.raises(ValueError):
            fn(N[:2], A[:2], p[:2], m[:3])
        with pytest.raises(TypeError, match="bool"):
            fn(N[0], A[0], p[0], m[0] > 0)
        with pytest.raises(ValueError):
            fn(N[0], A[0], p[0], mode="l2")
        with pytest.raises(ValueError):
            fn(N[0], A[0], p[0], min_norm=-1.0)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        normal_map_loss(N[0], A[0], p[0])                     # no CPU fallback behind the HIP name


def test_the_c_entries_validate_their_arguments(lib):
    """Reported before anything is enqueued: no GPU touched.  Host addresses stand in for device pointers."""
    buf = (C.c_double * 4096)()
    addr = (C.addressof(buf) + 15) & ~15                      # 16-byte aligned, as the workspace must be
    field = lambda n: (_lib.c_fp * _lib.MAX_POSE_ROWS)(*([addr] * n + [None] * (_lib.MAX_POSE_ROWS - n)))      # noqa: E731
    err = lambda: lib.bags_last_error()                                                                      # noqa: E731
    assert C.sizeof(_lib.BagsNormalMap) == 6 * 4 + 4 * 16 * 8
    make = lambda mode=0, H=8, W=8, n=2, mw=0.5, mn=0.1, have=2: _lib.BagsNormalMap(mode, H, W, n, mw, mn, field(have), field(have), field(have),     # noqa: E731
                                                                                    field(0))
    size = lib.bags_normal_map_workspace_size
    assert size(0, 8, 8) == 0 and size(17, 8, 8) == 0 and size(1, 0, 8) == 0 and size(1, 65536, 65536) == 0
    assert size(2, 8, 8) >= 2 * 1 * 2 * 8 and size(16, 1080, 1920) > size(1, 1080, 1920) >= 64 * 2 * 8      # a row of 2 doubles per workgroup
    fwd = lambda a, ws=addr, nb=1 << 20, loss=addr, count=addr, stats=addr: lib.bags_normal_map_forward(C.byref(a), ws, nb, loss, count, stats, None)     # noqa: E731
    assert lib.bags_normal_map_forward(None, addr, 1 << 20, addr, addr, addr, None) == -1 and b"null struct" in err()
    assert fwd(make(mode=2)) == -1 and b"unknown mode" in err()
    for n in (0, 17):
        assert fwd(make(n=n)) == -1 and b"n_rows" in err()
    assert fwd(make(H=0)) == -1 and b"empty image" in err()
    assert fwd(make(H=65536, W=65536)) == -1 and b"2^31" in err()
    assert fwd(make(mw=float("nan"))) == -1 and b"min_weight" in err()
    assert fwd(make(mn=-0.1)) == -1 and b"min_norm" in err()
    assert fwd(make(have=1)) == -1 and b"null normal[1]" in err()          # fewer pointers than n_rows says
    assert fwd(make(), loss=None) == -1 and b"null loss" in err()
    assert fwd(make(), ws=None) == -1 and b"workspace" in err()
    assert fwd(make(), nb=8) == -1 and b"workspace" in err()
    assert fwd(make(), ws=addr + 8) == -1 and b"16-byte" in err()
    assert fwd(make(), stats=addr + 4) == -1 and b"8-byte" in err()
    bwd = lambda a, stats=addr, g=addr, gn=field(2): lib.bags_normal_map_backward(C.byref(a), stats, g, gn, None)                   # noqa: E731
    assert bwd(make(), stats=None) == -1 and b"null stats" in err()
    assert bwd(make(), g=None) == -1 and b"null g_loss" in err()
    assert bwd(make(mode=7)) == -1 and b"unknown mode" in err()
    assert bwd(make(), gn=field(0)) == 0 and bwd(make(), gn=None) == 0      # nothing wanted: a successful no-op
