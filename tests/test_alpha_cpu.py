"""CPU checks of bags_raster.alpha_loss: the PyTorch statement against values computed by hand on a 2 x 3 map in all four modes;
what the case generator of tests/alpha_cases.py promises; gradcheck; the derivative rule at the clamp and at A == t; a view without
a usable pixel; the argument errors of the Python names; the C entries' validation through the library, without a GPU."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import alpha_cases as M
from bags_raster import _lib, alpha_loss, alpha_loss_torch

F32, F64 = torch.float32, torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


# ------------------------------------------------------------------------------------------------------------------ by hand
def _by_hand(mode):
    """A 2 x 3 map with eps = 1/8: a pixel clamped at each end, three inside (one of them at A == t), one NaN; weights 1, 2, 1, 1/2,
    1, 1: cnt = 5.5.  (loss, [dL/dA of the six pixels]) from math.log alone."""
    H_ = lambda a: -(a * math.log(a) + (1 - a) * math.log(1 - a))                              # noqa: E731
    cnt = 5.5
    if mode == "bce":         # t = 0, 1, .5, 1, 1 ;  a = 1/8, 1/4, 1/2, 3/4, 7/8
        loss = (-math.log(0.875) + 2 * -math.log(0.25) + math.log(2.0) + 0.5 * -math.log(0.75) + -math.log(0.875)) / cnt
        grad = [0.0, 2 / cnt * (0.25 - 1) / (0.25 * 0.75), 0.0, 0.5 / cnt * (0.75 - 1) / (0.75 * 0.25), 0.0, 0.0]
    elif mode == "entropy":
        loss = (H_(0.125) + 2 * H_(0.25) + H_(0.5) + 0.5 * H_(0.75) + H_(0.875)) / cnt
        grad = [0.0, 2 / cnt * math.log(3.0), 0.0, 0.5 / cnt * math.log(1 / 3), 0.0, 0.0]
    elif mode == "l1":        # |A - t| = 0, 3/4, 0, 1/4, 0
        loss = (2 * 0.75 + 0.5 * 0.25) / cnt
        grad = [0.0, -2 / cnt, 0.0, -0.5 / cnt, 0.0, 0.0]
    else:
        loss = (2 * 0.5625 + 0.5 * 0.0625) / cnt
        grad = [0.0, 2 / cnt * 2 * -0.75, 0.0, 0.5 / cnt * 2 * -0.25, 0.0, 0.0]
    return loss, grad


@pytest.mark.parametrize("mode", M.MODES)
@pytest.mark.parametrize("dtype", (F64, F32))
def test_the_statement_against_values_computed_by_hand(mode, dtype):
    A = torch.tensor([[0.0, 0.25, 0.5], [0.75, 1.0, float("nan")]], dtype=dtype).requires_grad_()
    t = None if mode == "entropy" else torch.tensor([[0.0, 1.0, 0.5], [1.0, 1.0, 0.0]], dtype=dtype)
    m = torch.tensor([[1.0, 2.0, 1.0], [0.5, 1.0, 1.0]], dtype=dtype)
    loss, count = alpha_loss_torch(A[None], t, m, mode=mode, eps=0.125)
    assert loss.shape == (1,) and count.shape == (1,) and loss.dtype == dtype and not count.requires_grad
    (g,) = torch.autograd.grad(loss.sum(), A)
    want_l, want_g = _by_hand(mode)
    tol = 1e-14 if dtype == F64 else 1e-6
    assert count.item() == 5.5 and abs(loss.item() - want_l) <= tol * (1 + abs(want_l))
    assert torch.allclose(g.reshape(-1).double(), torch.tensor(want_g, dtype=F64), rtol=tol, atol=tol)
    assert (g.reshape(-1)[[0, 2, 4, 5]] == 0).all() if mode != "entropy" else (g.reshape(-1)[[0, 4, 5]] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ the generator
def test_what_the_generator_promises():
    """Every generic case counts something in every view; from 33 x 70 on it has pixels inside and pixels clamped at both ends;
    apart from the placed ones every A is MARGIN / 2 or more away from lo and hi."""
    for (H, W) in M.SIZES:
        for V in M.VIEWS:
            c = M.case("generic", H, W, V)
            lo, hi = c["eps"], 1.0 - c["eps"]
            for mode in M.MODES:
                for masked in (False, True):
                    _, n, _ = M.forward_backward(alpha_loss_torch, "generic", H, W, V, mode, masked, F64, "cpu")
                    assert (n > 0).all(), (H, W, V, mode, masked)
            for v in range(V):
                A, m = c["weights"][v].double(), c["mask"][v]
                assert ((A == 0) | (A == 1) | (((A - lo).abs() >= 1e-3) & ((A - hi).abs() >= 1e-3))).all()
                if H * W >= 33 * 70:
                    for keep in (torch.ones_like(m, dtype=torch.bool), m > 0):
                        a = A[0][keep]
                        assert (a <= lo).any() and (a >= hi).any() and ((a > lo) & (a < hi)).any()
                        assert (a == 0).any() and (a == 1).any()
    for name in ("holes", "edges"):
        for (H, W) in M.SIZES[2:]:
            c = M.case(name, H, W, 5)
            lo, hi = c["eps"], 1.0 - c["eps"]
            for v in range(5):
                A = c["weights"][v].double().reshape(-1)[(7 if name == "edges" else 0):]
                A = A[torch.isfinite(A)]
                assert (((A - lo).abs() >= 1e-3) & ((A - hi).abs() >= 1e-3)).all()
    assert M.case("generic", 5, 7, 5)["weights"][0] is M.case("generic", 5, 7, 5)["weights"][0]            # cached, never rebuilt


def test_float32_and_float64_decide_alike():
    for name in M.CASES:
        for mode in M.MODES:
            for (H, W) in ((5, 7), (33, 70)):
                l64, n64, g64 = M.forward_backward(alpha_loss_torch, name, H, W, 5, mode, True, F64, "cpu")
                l32, n32, g32 = M.forward_backward(alpha_loss_torch, name, H, W, 5, mode, True, F32, "cpu")
                assert l32.dtype == F32 and torch.isfinite(l64).all() and torch.isfinite(l32).all()
                assert ((l32.double() - l64).abs() <= 1e-5 * (1 + l64.abs())).all() and ((n32.double() - n64).abs() <= 1e-5 * (1 + n64)).all()
                for a, b in zip(g32, g64):
                    assert torch.isfinite(a).all() and torch.isfinite(b).all() and torch.equal(a == 0, b == 0)


def test_gradcheck():
    c = M.case("generic", 5, 7, 5)
    A = torch.stack(c["weights"][:2]).double().requires_grad_()
    t, m = [x.double() for x in c["target"][:2]], [x.double() for x in c["mask"][:2]]
    for mode in M.MODES:
        tt = None if mode == "entropy" else t
        assert torch.autograd.gradcheck(lambda A: alpha_loss_torch(list(A), tt, m, mode=mode, eps=M.EPS)[0], (A,))


# ------------------------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("dtype", (F64, F32))
def test_the_derivative_rule_at_the_edges(dtype):
    """Zero at and beyond the clamp in bce and entropy, not zero one float32 step inside it; sign(0) = 0 in l1."""
    inside = torch.tensor(M.EDGES["inside"])
    same = M.EDGES["equal_target"]
    for mode in M.MODES:
        _, _, g = M.forward_backward(alpha_loss_torch, "edges", 5, 7, 5, mode, True, dtype, "cpu")
        for v in range(5):
            first = g[v].reshape(-1)[:7]
            if mode in M.CLAMPED:
                assert torch.equal(first[:same] != 0, inside[:same]), (mode, first)
                assert first[same].abs() <= 1e-12 if mode == "bce" else first[same] != 0      # a == t: autograd's two terms cancel to an ulp
            elif mode == "l1":
                assert first[same] == 0 and (first[:same] != 0).all()
                assert torch.equal(first[:same].sign(), -M.cotangent(5)[v].sign() * torch.tensor([1.0, 1, 1, -1, -1, -1]).to(first))
            else:
                assert first[same] == 0 and (first[:same] != 0).all()


def test_a_view_without_a_usable_pixel_is_zero_not_nan():
    for mode in M.MODES:
        for masked in (False, True):
            l, n, g = M.forward_backward(alpha_loss_torch, "empty", 5, 7, 5, mode, masked, F64, "cpu")
            assert torch.isfinite(l).all() and (l[0::2] == 0).all() and (n[0::2] == 0).all() and (n[1::2] > 0).all()
            assert all(torch.isfinite(x).all() for x in g) and all((x == 0).all() for x in g[0::2]) and all(x.abs().max() > 0 for x in g[1::2])


def test_holes_get_exact_zero_gradients():
    H, W = 33, 70
    kind = M.hole_kind(H, W)
    for mode in M.MODES:
        for masked in (False, True):
            l, n, g = M.forward_backward(alpha_loss_torch, "holes", H, W, 5, mode, masked, F64, "cpu")
            bad = torch.isin(kind, torch.tensor(M.unusable_kinds(mode, masked)))
            assert torch.isfinite(l).all() and (n > 0).all()
            for v in range(5):
                assert torch.isfinite(g[v]).all() and (g[v][0][bad] == 0).all() and (g[v][0][~bad] != 0).all()


def test_argument_errors():
    c = M.case("generic", 5, 7, 5)
    A, t, m = c["weights"], c["target"], c["mask"]
    for fn in (alpha_loss_torch, alpha_loss):
        with pytest.raises(ValueError, match="entropy"):
            fn(A[0], t[0], mode="entropy")
        for mode in ("bce", "l1", "l2"):
            with pytest.raises(ValueError, match="needs a target"):
                fn(A[0], None, mode=mode)
        with pytest.raises(TypeError, match=r"mask\.float\(\)"):
            fn(A[0], t[0], m[0] > 0)
        for eps in (0.0, 0.5, -1e-3, 0.7, float("nan")):
            with pytest.raises(ValueError, match="eps"):
                fn(A[0], t[0], eps=eps)
        with pytest.raises(ValueError, match="mode"):
            fn(A[0], t[0], mode="cos")
        with pytest.raises(ValueError):
            fn(A[0][0, :, :3], t[0])                          # another size
        with pytest.raises(ValueError):
            fn(A[:2], t[:3])                                  # more targets than views
        with pytest.raises(ValueError):
            fn(A[:2], t[:2], m[:3])
        with pytest.raises(ValueError):
            fn(torch.zeros(3, 5, 7), t[0])                    # not (H,W) or (1,H,W)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        alpha_loss(A[0], t[0])                                # no CPU fallback behind the HIP name


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_the_abi_is_additive(lib):
    assert lib.bags_abi_version() == 11 == _lib.ABI_VERSION
    assert C.sizeof(_lib.BagsAlpha) == 6 * 4 + 3 * 16 * 8
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    define = lambda name: re.search(r"#define\s+%s\s+(.+?)\s*(?:/\*|$)" % name, header, re.M).group(1)       # noqa: E731
    groups, stats, rows = int(define("BAGS_ALPHA_GROUPS")), int(define("BAGS_ALPHA_STATS")), int(define("BAGS_MAX_POSE_ROWS"))
    assert define("BAGS_ALPHA_WORKSPACE_BYTES") == "(BAGS_MAX_POSE_ROWS * BAGS_ALPHA_GROUPS * BAGS_ALPHA_STATS * 8)"
    assert (_lib.ALPHA_GROUPS, _lib.ALPHA_STATS, _lib.MAX_POSE_ROWS) == (groups, stats, rows)
    assert _lib.ALPHA_WORKSPACE_BYTES == rows * groups * stats * 8
    assert groups <= 256 and groups & (groups - 1) == 0
    assert [int(define("BAGS_ALPHA_" + n)) for n in ("BCE", "L1", "L2", "ENTROPY")] == [0, 1, 2, 3] == \
        [_lib.ALPHA_BCE, _lib.ALPHA_L1, _lib.ALPHA_L2, _lib.ALPHA_ENTROPY]
    assert not [n for n in _lib.SYMBOLS if n.startswith("bags_alpha_") and n.endswith("_workspace_size")]
    assert {n for n in _lib.SYMBOLS if n.startswith("bags_alpha_")} == {"bags_alpha_forward", "bags_alpha_backward"}
    assert not hasattr(lib, "bags_alpha_workspace_size")


def test_the_c_entries_validate_their_arguments(lib):
    """Reported before anything is enqueued: no GPU touched.  Host addresses stand in for device pointers."""
    need = _lib.ALPHA_WORKSPACE_BYTES
    buf = (C.c_double * (need // 8 + 64))()
    addr = (C.addressof(buf) + 15) & ~15                      # 16-byte aligned, as the workspace must be
    field = lambda n: (_lib.c_fp * _lib.MAX_POSE_ROWS)(*([addr] * n + [None] * (_lib.MAX_POSE_ROWS - n)))      # noqa: E731
    err = lambda: lib.bags_last_error()                                                                      # noqa: E731
    make = lambda mode=0, H=8, W=8, n=2, lo=1e-4, hi=1 - 1e-4, have=2, targets=2: _lib.BagsAlpha(mode, H, W, n, lo, hi, field(have),   # noqa: E731
                                                                                              field(targets), field(0))
    fwd = lambda a, ws=addr, nb=need, loss=addr, count=addr, stats=addr: lib.bags_alpha_forward(C.byref(a), ws, nb, loss, count, stats, None)     # noqa: E731
    assert lib.bags_alpha_forward(None, addr, need, addr, addr, addr, None) == -1 and b"null struct" in err()
    for mode in (-1, 4):
        assert fwd(make(mode=mode)) == -1 and b"unknown mode" in err()
    for n in (0, 17):
        assert fwd(make(n=n)) == -1 and b"n_rows" in err()
    assert fwd(make(H=0)) == -1 and b"empty image" in err()
    assert fwd(make(H=65536, W=32768)) == -1 and b"2^31" in err()
    for lo, hi in ((0.0, 0.9), (0.6, 0.4), (0.1, 1.0), (float("nan"), 0.9)):
        assert fwd(make(lo=lo, hi=hi)) == -1 and b"lo < hi" in err()
    assert fwd(make(have=1)) == -1 and b"null weights[1]" in err()         # fewer pointers than n_rows says
    assert fwd(make(targets=1)) == -1 and b"null target[1]" in err()
    assert fwd(make(mode=3, targets=0), nb=need - 1) == -1 and b"workspace" in err()      # entropy: no target wanted; the size comes next
    assert fwd(make(), loss=None) == -1 and b"null loss" in err()
    assert fwd(make(), ws=None) == -1 and b"workspace" in err()
    assert fwd(make(), nb=need - 1) == -1 and (b"workspace of %d bytes (got %d)" % (need, need - 1)) in err()
    for off in (4, 8):
        assert fwd(make(), ws=addr + off, nb=need) == -1 and b"16-byte" in err()
    assert fwd(make(), stats=addr + 4) == -1 and b"8-byte" in err()
    bwd = lambda a, stats=addr, g=addr, gw=field(2): lib.bags_alpha_backward(C.byref(a), stats, g, gw, None)                        # noqa: E731
    assert bwd(make(), stats=None) == -1 and b"null stats" in err()
    assert bwd(make(), g=None) == -1 and b"null g_loss" in err()
    assert bwd(make(mode=7)) == -1 and b"unknown mode" in err()
    assert bwd(make(have=1)) == -1 and b"null weights[1]" in err()
    assert bwd(make(), gw=field(0)) == 0 and bwd(make(), gw=None) == 0      # nothing wanted: a successful no-op
