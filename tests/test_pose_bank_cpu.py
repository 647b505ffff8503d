"""No-GPU checks of the camera bank (bags_raster/pose_bank.py; bags_pose_bank_forward / bags_pose_bank_backward /
bags_pose_adam_step of include/bags_raster.h): the boundary, the argument validation, and the host path, which is PoseCamera's own
getters row by row."""
import ctypes as C
import os
import re

import pytest
import torch

import bags_raster
from bags_raster import _lib
from bags_raster import camera as cam
from bags_raster.pose_bank import PoseAdam, PoseBank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bags_pose_bank_forward", "bags_pose_bank_backward", "bags_pose_adam_step")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _cameras(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        c = cam.PoseCamera(cam.quaternion_to_rotation(torch.randn(4, generator=g)), torch.randn(3, generator=g) + torch.tensor([0.0, 0.0, 4.0]),
                           1.1 - 0.1 * i, 0.7 + 0.05 * i, 64 + i, 48 - i, znear=0.01 * (i + 1), zfar=100.0 + i)
        with torch.no_grad():
            c.delta_quaternion.copy_(0.05 * torch.randn(4, generator=g))
            c.delta_translation.copy_(0.1 * torch.randn(3, 1, generator=g))
            c.learnable_fovx.add_(0.03); c.learnable_fovy.sub_(0.02)
        out.append(c)
    return out


def test_header_symbols_structs_and_abi(lib):
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    for text in ("#define BAGS_MAX_POSE_ROWS 16", "} BagsPoseBank;", "} BagsPoseAdamGroup;", "} BagsPoseAdamArgs;", "#define BAGS_ABI_VERSION 11"):
        assert text in header, text
    assert lib.bags_abi_version() == 11 == _lib.ABI_VERSION
    assert _lib.MAX_POSE_ROWS == 16
    assert C.sizeof(_lib.BagsPoseBank) == 8 + 6 * 8 + 4 + 16 * 4 + 4 and _lib.BagsPoseBank.rows.offset == 60
    assert C.sizeof(_lib.BagsPoseAdamGroup) == 12
    assert C.sizeof(_lib.BagsPoseAdamArgs) == 8 + 4 * 8 + 3 * 8 + 16 * 4 + 16 * 3 * 12 and _lib.BagsPoseAdamArgs.groups.offset == 128
    assert "PoseBank" in bags_raster.__all__ and "PoseAdam" in bags_raster.__all__ and bags_raster.PoseBank is PoseBank


def _bank_struct(N=4, rows=(0,), tables=(8, 8, 8, 8)):
    """Non-NULL table addresses that are never read: every call below must be rejected on the host before any launch."""
    return _lib.BagsPoseBank(N, *[t or None for t in tables], None, None, len(rows), (C.c_int32 * 16)(*rows))


def _rejected(lib, rc, text):
    assert rc != 0
    msg = lib.bags_last_error().decode()
    assert text in msg, msg


def test_c_entries_reject_bad_arguments(lib):
    out = [C.c_void_p(8)] * 4
    fwd = lambda b: lib.bags_pose_bank_forward(b, *out, None)
    bwd = lambda b, gl=16, gr=None, gs=None: lib.bags_pose_bank_backward(b, None, None, None, None, gl, gr, gs, None)
    for call in (fwd, bwd):
        _rejected(lib, call(None), "null struct")
        _rejected(lib, call(_bank_struct(rows=())), "n_rows 0 not in 1..16")
        b = _bank_struct(N=40, rows=tuple(range(16)))
        b.n_rows = 17
        _rejected(lib, call(b), "n_rows 17 not in 1..16")
        _rejected(lib, call(_bank_struct(rows=(1, 4))), "rows[1] = 4 is not in [0, 4)")
        _rejected(lib, call(_bank_struct(rows=(-1,))), "rows[0] = -1 is not in [0, 4)")
        _rejected(lib, call(_bank_struct(rows=(2, 0, 2))), "row 2 is listed twice")
        _rejected(lib, call(_bank_struct(N=0)), "N 0 < 1")
        for k in range(4):
            _rejected(lib, call(_bank_struct(tables=tuple(0 if i == k else 8 for i in range(4)))), "tables must be given")
    _rejected(lib, lib.bags_pose_bank_forward(_bank_struct(), None, *out[1:], None), "null output")
    _rejected(lib, bwd(_bank_struct(), gl=None), "null grad_leaves")
    _rejected(lib, bwd(_bank_struct(), gl=8), "must not be the leaves table")
    _rejected(lib, bwd(_bank_struct(), gr=8), "without a global_rotation")
    _rejected(lib, bwd(_bank_struct(), gs=8), "without a global_translation_scale")

    def adam(N=4, rows=(0,), tables=(8, 8, 8, 8)):
        return _lib.BagsPoseAdamArgs(N, len(rows), *[t or None for t in tables], 0.9, 0.999, 1e-8, (C.c_int32 * 16)(*rows))
    step = lambda a: lib.bags_pose_adam_step(a, None)
    _rejected(lib, step(None), "null struct")
    _rejected(lib, step(adam(rows=())), "n_rows 0 not in 1..16")
    _rejected(lib, step(adam(rows=(0, 7))), "rows[1] = 7 is not in [0, 4)")
    _rejected(lib, step(adam(rows=(3, 3))), "row 3 is listed twice")
    for k in range(4):
        _rejected(lib, step(adam(tables=tuple(0 if i == k else 8 for i in range(4)))), "tables must be given")


def test_python_rejects_bad_rows_and_a_missing_gradient():
    bank = PoseBank.from_cameras(_cameras(3))
    with pytest.raises(ValueError, match="row 1 is listed twice"):
        bank.get_matrices([1, 0, 1])
    with pytest.raises(ValueError, match=r"row 3 is not in \[0, 3\)"):
        bank.get_matrices([0, 3])
    with pytest.raises(ValueError, match=r"row -1 is not in \[0, 3\)"):
        bank.camera(-1)
    with pytest.raises(ValueError, match="the row list is empty"):
        bank.get_matrices([])
    opt = PoseAdam(bank, 1e-3, 1e-3, 1e-4)
    with pytest.raises(RuntimeError, match="has no .grad"):
        opt.step([0])
    with pytest.raises(ValueError, match="row 2 is listed twice"):
        opt.step([2, 2])
    bank.leaves.grad = torch.zeros_like(bank.leaves)
    with pytest.raises(RuntimeError, match="runs only on an AMD GPU"):          # no CPU fallback
        opt.step([0])
    assert not opt.step_count.any()
    with pytest.raises(ValueError, match="znear < zfar"):
        PoseBank(torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3), 1.0, 1.0, 8, 8, znear=[0.1, 2.0], zfar=1.0)
    with pytest.raises(ValueError, match="FoVx has 3 entries for 2 cameras"):
        PoseBank(torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3), [1.0, 1.0, 1.0], 1.0, 8, 8)


@pytest.mark.parametrize("align", [False, True])
def test_host_bank_is_pose_cameras_getters_row_by_row(align):
    cams = _cameras(4)
    bank = PoseBank.from_cameras(cams)
    assert [n for n, _ in bank.named_parameters()] == ["leaves"] and bank.leaves.shape == (4, 9)
    assert sorted(n for n, _ in bank.named_buffers()) == ["init_quaternion", "init_translation", "near_far"]
    g = torch.Generator().manual_seed(11)
    mk = lambda: (cam.quaternion_to_rotation(torch.tensor([1.0, 0.02, -0.03, 0.01])).requires_grad_(True), torch.tensor(1.3, requires_grad=True))
    ga0, ga1 = (mk(), mk()) if align else ((None, None), (None, None))
    rows = [2, 0, 3]
    cots = [torch.randn(3, 4, 4, generator=g), torch.randn(3, 4, 4, generator=g), torch.randn(3, 4, 4, generator=g), torch.randn(3, 3, generator=g)]
    got = bank.get_matrices(rows, *ga0)
    assert [tuple(t.shape) for t in got] == [(3, 4, 4)] * 3 + [(3, 3)]
    want = [cams[r].get_matrices(*ga1) for r in rows]
    for k in range(4):
        for v in range(3):
            assert torch.equal(got[k][v], want[v][k]), (k, v)
    sum((c * o).sum() for c, o in zip(cots, got)).backward()
    sum((c[v] * want[v][k]).sum() for v in range(3) for k, c in enumerate(cots)).backward()
    for r in range(4):
        leaf = torch.cat([torch.zeros(1) if t.grad is None else t.grad.reshape(-1) for t in cams[r].pose_leaves()]) if r in rows else torch.zeros(9)
        assert torch.allclose(bank.leaves.grad[r], leaf, rtol=1e-6, atol=1e-7), r      # autograd's accumulation order differs, not the chain
    assert not bank.leaves.grad[1].any()
    if align:
        for a, b in zip(ga0, ga1):
            assert torch.allclose(a.grad, b.grad, rtol=1e-5, atol=1e-6)
    one = bank.camera(3)
    assert (one.image_width, one.image_height, one.FoVx, one.FoVy) == (cams[3].image_width, cams[3].image_height, cams[3].FoVx, cams[3].FoVy)
    for a, b in zip(one.get_matrices(*ga0), cams[3].get_matrices(*ga1)):
        assert torch.equal(a, b)


def test_from_cameras_then_export_round_trips():
    cams = _cameras(3)
    bank = PoseBank.from_cameras(cams)
    assert len(bank) == 3
    for i, c in enumerate(cams):
        e = bank.export(i)
        assert isinstance(e, cam.PoseCamera)
        sd, want = e.state_dict(), c.state_dict()
        assert list(sd) == list(want)
        for k in want:
            assert sd[k].shape == want[k].shape and torch.equal(sd[k], want[k]), k
        for k in ("image_width", "image_height", "FoVx", "FoVy", "znear", "zfar"):
            assert getattr(e, k) == getattr(c, k), k
        assert all(p.requires_grad for p in e.pose_leaves())
    again = PoseBank.from_cameras([bank.export(i) for i in range(3)])
    for (n, a), (_, b) in zip(sorted(bank.state_dict().items()), sorted(again.state_dict().items())):
        assert torch.equal(a, b), n
    # direct construction states the same cameras
    R = torch.stack([cam.quaternion_to_rotation(c.init_quaternion).t() for c in cams])
    direct = PoseBank(R, torch.stack([c.init_translation.reshape(3) for c in cams]), [c.FoVx for c in cams], [c.FoVy for c in cams],
                      [c.image_width for c in cams], [c.image_height for c in cams], znear=[c.znear for c in cams], zfar=[c.zfar for c in cams])
    assert torch.allclose(direct.init_quaternion, bank.init_quaternion, atol=1e-6) and torch.equal(direct.near_far, bank.near_far)
    assert not direct.leaves[:, :7].any() and torch.equal(direct.leaves[:, 7], torch.tensor([c.FoVx for c in cams]))
    assert direct.image_width == bank.image_width and direct.FoVy == bank.FoVy


def test_pose_adam_state_dict_round_trips():
    bank = PoseBank.from_cameras(_cameras(5))
    opt = PoseAdam(bank, 1e-3, 2e-3, 3e-4, betas=(0.8, 0.99), eps=1e-10)
    g = torch.Generator().manual_seed(2)
    opt.exp_avg.copy_(torch.randn(5, 9, generator=g)); opt.exp_avg_sq.copy_(torch.rand(5, 9, generator=g))
    opt.step_count[3] = torch.tensor([3, 3, 2]); opt.step_count[0, 1] = 1000
    opt.lr_translation = 5e-4                                   # the schedule is an assignment
    state = opt.state_dict()
    assert state["step"].dtype == torch.int64 and state["step"].device.type == "cpu" and state["step"].shape == (5, 3)
    other = PoseAdam(PoseBank.from_cameras(_cameras(5)), 0.0, 0.0, 0.0)
    other.load_state_dict(state)
    assert torch.equal(other.step_count, opt.step_count) and other.step_count is not state["step"]
    assert torch.equal(other.exp_avg, opt.exp_avg) and torch.equal(other.exp_avg_sq, opt.exp_avg_sq)
    assert (other.lr_rotation, other.lr_translation, other.lr_fov, other.betas, other.eps) == (1e-3, 5e-4, 3e-4, (0.8, 0.99), 1e-10)
    state["step"][3, 0] = 99                                    # a copy both ways
    assert opt.step_count[3, 0] == 3 and other.step_count[3, 0] == 3
    with pytest.raises(ValueError, match="exp_avg has shape"):
        PoseAdam(PoseBank.from_cameras(_cameras(4)), 0.0, 0.0, 0.0).load_state_dict(state)
