"""No-GPU checks of the cubemap stitch: the inputs of tests/test_resample_faces_gpu.py (tests/faces_cases.py) hold what its bars
rest on, the PyTorch statement of the function agrees with grid_sample where there is one face, and the boundary (struct layout,
ABI, argument errors) answers before anything is enqueued."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import bags_raster
import faces_cases as FC
from bags_raster import _lib, cube_face_matrices, resample_faces, resample_faces_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_borderline_pixels_are_rare(name):
    """At most 1 % of a case's pixels are within 1e-4 of a face decision, and the float32 PyTorch route decides no pixel with a
    larger margin differently from float64."""
    m = FC.case_margin(name)
    share = float((m < FC.MARGIN).double().mean())
    c = FC.make_case(name)
    idx64 = FC.reference(name)[1]
    idx32 = resample_faces_torch(c["faces"], c["ctrl"], c["mats"], c["flow_hw"], c["crop_hw"])[1]
    flips = idx32 != idx64
    print(f"{name}: share of pixels with margin < {FC.MARGIN:g}: {share:.5f}; float32 flips {int(flips.sum())}")
    assert share <= FC.MAX_BORDERLINE, share
    assert not bool((flips & (m >= FC.MARGIN)).any())
    assert idx64.dtype == torch.int8 and tuple(idx64.shape) == tuple(c["crop_hw"])


def _tiles_with(idx, face):
    """Number of 16x16 output tiles that hold a pixel of ``face``; and the largest number of faces in one tile."""
    Hc, Wc = idx.shape
    n, most = 0, 0
    for y in range(0, Hc, 16):
        for x in range(0, Wc, 16):
            t = idx[y:y + 16, x:x + 16]
            n += int((t == face).any())
            most = max(most, len(set(t[t >= 0].tolist())))
    return n, most


def test_cases_exercise_what_they_are_for():
    used = lambda name: [int((FC.reference(name)[1] == f).sum()) for f in range(-1, FC.CASES[name]["faces"])]
    for name in ("all_faces", "larger", "all_faces_c1", "all_faces_c4"):
        assert used(name)[0] == 0 and min(used(name)[1:]) > 0, (name, used(name))       # every pixel covered, all five faces used
    assert _tiles_with(FC.reference("all_faces")[1], 0)[1] >= 3                           # a tile at a cube corner: three faces
    u = used("overlap")                                                                   # up and down are never chosen
    assert u[0] == 0 and min(u[1:4]) > 0 and u[4] == 0 and u[5] == 0, u
    # list order decides inside the overlap: pixels where two faces are valid exist, and they go to the first
    c = FC.make_case("overlap")
    uu, vv, cc = FC.coords(c["ctrl"], c["mats"], c["flow_hw"], c["crop_hw"])
    valid = (cc > 0) & (uu.abs() <= 1) & (vv.abs() <= 1)
    both = valid.sum(0) >= 2
    assert int(both.sum()) > 20
    assert torch.equal(FC.reference("overlap")[1][both].long(), valid.long().argmax(0)[both])
    u = used("hole")
    assert u[0] > 100 and u[1] > 100 and u[2] > 100, u
    n_front, _ = _tiles_with(FC.reference("minification")[1], 0)                          # one 16x16 source tile per face ...
    assert FC.CASES["minification"]["S"] == 16 and n_front > 2 * 32, n_front             # ... under far more than 32 output tiles


def test_one_face_and_the_identity_is_grid_sample():
    g = torch.Generator().manual_seed(0)
    for dtype in (torch.float32, torch.float64):
        img = torch.rand(3, 30, 40, generator=g, dtype=dtype)
        ctrl = torch.rand(6, 8, 2, generator=g, dtype=dtype) * 3.2 - 1.6
        out, idx = resample_faces_torch([img], ctrl, torch.eye(3).unsqueeze(0), (33, 44), (30, 40))
        flow = F.interpolate(ctrl.permute(2, 0, 1).unsqueeze(0), size=(33, 44), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
        flow = flow[1:31, 2:42]
        ref = F.grid_sample(img.unsqueeze(0), flow.unsqueeze(0), mode="bilinear", padding_mode="zeros", align_corners=True)[0]
        inside = (flow[..., 0].abs() <= 1) & (flow[..., 1].abs() <= 1)
        assert out.dtype == dtype and torch.equal(idx == 0, inside) and torch.equal(idx == -1, ~inside)
        assert 0.2 < float(inside.double().mean()) < 0.95
        assert torch.equal(out[:, inside], ref[:, inside]) and not bool(out[:, ~inside].any())
        # a given map is replayed, not decided again: everything to face 0 is the plain grid_sample, padding and all
        all0 = resample_faces_torch([img], ctrl, torch.eye(3).unsqueeze(0), (33, 44), (30, 40), face_index=torch.zeros(30, 40, dtype=torch.int8))
        assert torch.equal(all0[0], ref)


@pytest.mark.parametrize("name", ["all_faces", "overlap", "hole"])
def test_reference_gradients_are_finite(name):
    out, idx, g_faces, g_ctrl = FC.reference(name)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g_ctrl).all()) and float(g_ctrl.abs().max()) > 0
    for f, g in enumerate(g_faces):
        assert bool(torch.isfinite(g).all())
        assert (float(g.abs().max()) > 0) == bool((idx == f).any())                  # a face no pixel chose: exact zeros
    assert not bool(out[:, idx < 0].any())
    # the reference does not bless itself: it is its own replay, and a wrong answer is far outside the bars
    again = FC.reference(name, idx)
    assert FC.errors(again, (out, idx, g_faces, g_ctrl)) == (0.0, 0.0, 0.0)
    off = FC.errors((out * (1 + 1e-3), idx, [g * (1 + 1e-2) for g in g_faces], g_ctrl * (1 + 1e-2)), again)
    assert all(o > b for o, b in zip(off, FC.bars(again))), (off, FC.bars(again))


def test_cube_face_matrices():
    R, M = cube_face_matrices((1.3, 0.8), 1.05)
    assert R.shape == M.shape == (5, 3, 3) and R.dtype == M.dtype == torch.float64
    eye = torch.eye(3, dtype=torch.float64)
    for f in range(5):
        assert torch.equal(R[f] @ R[f].T, eye) and float(torch.linalg.det(R[f])) == 1.0
    # x right, y down, z forward: the optical axis of each face in the front camera's frame
    axes = torch.tensor([[0, 0, 1], [-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0]], dtype=torch.float64)
    for f in range(5):
        assert torch.equal(R[f] @ axes[f], torch.tensor([0, 0, 1], dtype=torch.float64))
    assert torch.equal(R[1] @ axes[0], torch.tensor([1.0, 0, 0], dtype=torch.float64))     # the front is to the left face's right
    assert torch.equal(R[3] @ axes[0], torch.tensor([0, 1.0, 0], dtype=torch.float64))     # ... and below the up face's centre
    D0 = torch.diag(torch.tensor([1.3, 0.8, 1.0], dtype=torch.float64))
    Df = torch.diag(torch.tensor([1 / 1.05, 1 / 1.05, 1.0], dtype=torch.float64))
    assert torch.allclose(M, Df @ R @ D0, rtol=0, atol=1e-15)
    assert torch.equal(cube_face_matrices(1.0)[1], R)
    # 90 degree faces tile the cube: every ray of the front half space lands in at least one face
    d = torch.randn(2000, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    d[:, 2] = d[:, 2].abs() + 1e-3
    p = torch.einsum("fij,nj->fni", R, d)
    valid = (p[..., 2] > 0) & (p[..., 0].abs() <= p[..., 2]) & (p[..., 1].abs() <= p[..., 2])
    assert bool(valid.any(0).all())


def test_symbols_struct_and_abi(lib):
    header = open(os.path.join(ROOT, "include", "bags_raster.h")).read()
    for name in ("bags_resample_faces_workspace_size", "bags_resample_faces_forward", "bags_resample_faces_backward"):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert re.search(r"#define\s+BAGS_MAX_FACES\s+8\b", header) and _lib.MAX_FACES == 8
    # typedef struct BagsFaces { int32_t n_faces, C, H, W; const float* image[8]; float mats[8][9]; }
    body = re.search(r"typedef struct BagsFaces \{(.*?)\} BagsFaces;", header, re.S).group(1)
    assert re.search(r"int32_t n_faces, C, H, W;", body) and re.search(r"const float\* image\[BAGS_MAX_FACES\];", body)
    assert re.search(r"float mats\[BAGS_MAX_FACES\]\[9\];", body)
    assert C.sizeof(_lib.BagsFaces) == 4 * 4 + 8 * 8 + 8 * 9 * 4
    assert _lib.BagsFaces.image.offset == 16 and _lib.BagsFaces.mats.offset == 16 + 64
    assert _lib.ABI_VERSION == 11 and lib.bags_abi_version() == 11 and re.search(r"#define\s+BAGS_ABI_VERSION\s+11\b", header)
    assert {"resample_faces", "resample_faces_torch", "cube_face_matrices"} <= set(bags_raster.__all__)
    size = lib.bags_resample_faces_workspace_size
    assert size(5, 1080, 1080, 1080, 1920) >= 1080 * 1920 * (8 + 16) + 5 * 68 * 68 * 33 * 4
    assert size(1, 24, 24, 40, 56) < size(5, 24, 24, 40, 56) < size(5, 24, 24, 80, 56)
    assert size(0, 24, 24, 40, 56) == 0 and size(9, 24, 24, 40, 56) == 0 and size(5, 0, 24, 40, 56) == 0 and size(5, 24, 24, 40, -1) == 0


def test_argument_errors(lib):
    """Every argument error comes back with its message before anything is enqueued: host memory stands in for device memory."""
    buf = (C.c_char * 64)()
    addr = C.addressof(buf)
    table = (_lib.c_fp * 8)(*([addr] * 8))

    def faces(n=5, Cn=3, H=24, W=24, null=None):
        f = _lib.BagsFaces(n, Cn, H, W)
        for i in range(8):
            f.image[i] = None if i == null else addr
        return f

    def both(f, h=9, w=13, Hf=44, Wf=60, Hc=40, Wc=56, ws=1 << 40):
        yield lib.bags_resample_faces_forward(C.byref(f), addr, h, w, Hf, Wf, Hc, Wc, addr, addr, None), b"resample_faces_forward"
        yield (lib.bags_resample_faces_backward(C.byref(f), addr, h, w, Hf, Wf, Hc, Wc, addr, addr, addr, ws, table, addr, None),
               b"resample_faces_backward")

    for kwargs, geom, what in [(dict(n=0), {}, b"n_faces 0 outside 1..8"), (dict(n=9), {}, b"n_faces 9 outside 1..8"),
                               (dict(Cn=5), {}, b"at most 4 channels"), (dict(null=2), {}, b"null image of face 2"),
                               (dict(Cn=0), {}, b"must be positive"), (dict(H=0), {}, b"must be positive"),
                               (dict(), dict(w=0), b"must be positive"), (dict(), dict(Hc=-1), b"must be positive"),
                               (dict(), dict(Hc=45), b"exceeds the flow size"), (dict(), dict(Wc=61), b"exceeds the flow size"),
                               (dict(W=32001), {}, b"too large")]:
        for rc, entry in both(faces(**kwargs), **geom):              # (a generator: each entry's message is read before the next call)
            assert rc == -1 and what in lib.bags_last_error() and entry in lib.bags_last_error(), (kwargs, geom, lib.bags_last_error())
    f = faces()
    assert lib.bags_resample_faces_forward(None, addr, 9, 13, 44, 60, 40, 56, addr, addr, None) == -1 and b"null BagsFaces" in lib.bags_last_error()
    assert lib.bags_resample_faces_forward(C.byref(f), None, 9, 13, 44, 60, 40, 56, addr, addr, None) == -1 and b"null pointer" in lib.bags_last_error()
    assert lib.bags_resample_faces_forward(C.byref(f), addr, 9, 13, 44, 60, 40, 56, addr, None, None) == -1 and b"null pointer" in lib.bags_last_error()
    need = lib.bags_resample_faces_workspace_size(5, 24, 24, 40, 56)
    rc = lib.bags_resample_faces_backward(C.byref(f), addr, 9, 13, 44, 60, 40, 56, addr, addr, addr, need - 1, table, addr, None)
    assert rc == -3 and (b"needs a workspace of %d bytes" % need) in lib.bags_last_error()
    assert lib.bags_resample_faces_backward(C.byref(f), addr, 9, 13, 44, 60, 40, 56, addr, addr, None, 0, table, None, None) == -3
    assert lib.bags_resample_faces_backward(C.byref(f), addr, 9, 13, 44, 60, 40, 56, None, addr, addr, 1 << 40, table, addr, None) == -1
    # no gradient asked for: nothing to do, and no workspace needed
    none = (_lib.c_fp * 8)()
    assert lib.bags_resample_faces_backward(C.byref(f), addr, 9, 13, 44, 60, 40, 56, addr, addr, None, 0, none, None, None) == 0
    assert lib.bags_resample_faces_backward(C.byref(f), addr, 9, 13, 44, 60, 40, 56, addr, addr, None, 0, None, None, None) == 0


def test_wrapper_refuses_before_the_gpu():
    c = FC.make_case("all_faces")
    with pytest.raises(RuntimeError, match="GPU tensor.*resample_faces_torch"):           # no silent CPU fallback
        resample_faces(c["faces"], c["ctrl"], c["mats"], c["flow_hw"], c["crop_hw"])
    with pytest.raises(RuntimeError, match="1..8 faces"):
        resample_faces([], c["ctrl"], c["mats"][:0], c["flow_hw"], c["crop_hw"])
    with pytest.raises(RuntimeError, match="1..8 faces"):
        resample_faces(c["faces"] * 2, c["ctrl"], torch.cat([c["mats"]] * 2), c["flow_hw"], c["crop_hw"])
    with pytest.raises(RuntimeError, match=r"mats \(5,3,3\)"):
        resample_faces(c["faces"], c["ctrl"], c["mats"][:4], c["flow_hw"], c["crop_hw"])
    with pytest.raises(RuntimeError, match=r"mats \(5,3,3\)"):
        resample_faces_torch(c["faces"], c["ctrl"], c["mats"][:4], c["flow_hw"], c["crop_hw"])
