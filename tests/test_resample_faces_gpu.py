"""The fused cubemap stitch (csrc/resample_faces.hip behind bags_resample_faces_forward / _backward) against its float64
statement in PyTorch.  The face a pixel belongs to is replayed in every reference from the kernel's own face_index, never decided
again; tests/faces_cases.py holds the cases and tests/test_resample_faces_cpu.py what they rest on."""
import pytest
import torch

import faces_cases as FC
from bags_raster import _lib as L
from bags_raster import resample_faces
from bags_raster.distortion import resample_image

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _run(name, need_faces=True, need_ctrl=True):
    c = FC.make_case(name)
    faces = [f.to(DEV).requires_grad_(need_faces) for f in c["faces"]]
    ctrl = c["ctrl"].to(DEV).requires_grad_(need_ctrl)
    out, idx = resample_faces(faces, ctrl, c["mats"], c["flow_hw"], c["crop_hw"])
    assert out.dtype == torch.float32 and idx.dtype == torch.int8 and not idx.requires_grad
    assert tuple(out.shape) == (FC.CASES[name]["C"],) + tuple(c["crop_hw"]) and tuple(idx.shape) == tuple(c["crop_hw"])
    out.backward(c["cot"].to(DEV))
    return out.detach(), idx, [f.grad for f in faces], ctrl.grad


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_stitch_matches_float64(name):
    out, idx, g_faces, g_ctrl = _run(name)
    idx_c = idx.cpu()
    # ---- the face map against the float64 reference's own choice
    idx64, m = FC.reference(name)[1], FC.case_margin(name)
    differ = idx_c != idx64
    print(f"{name}: {int(differ.sum())} of {differ.numel()} pixels choose another face than float64")
    assert not bool((differ & (m >= FC.MARGIN)).any())
    assert float(differ.double().mean()) <= FC.MAX_BORDERLINE
    # ---- the values against float64 GIVEN the kernel's map
    ref = FC.reference(name, idx_c)
    got = (out.cpu().double(), idx_c, [g.cpu().double() for g in g_faces], g_ctrl.cpu().double())
    err, err32, bars = FC.errors(got, ref), FC.errors(FC.float32_route(name, idx_c), ref), FC.bars(ref)
    print(f"{name}: image / dL/dfaces / dL/dctrl_flow max abs error: fused {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}; "
          f"float32 PyTorch {err32[0]:.2e} {err32[1]:.2e} {err32[2]:.2e}; bars {bars[0]:.2e} {bars[1]:.2e} {bars[2]:.2e}")
    assert err[0] <= bars[0] and err[1] <= bars[1] and err[2] <= bars[2], (err, bars)
    # uncovered pixels: zero in every channel; a face no pixel chose: exact zeros
    assert not bool(out[:, idx < 0].any())
    for f, g in enumerate(g_faces):
        assert bool((idx == f).any()) or not bool(g.any()), f
    if name == "hole":
        assert int((idx < 0).sum()) > 100
    if name == "overlap":
        assert not bool(g_faces[3].any()) and not bool(g_faces[4].any())


@pytest.mark.parametrize("name", ["all_faces", "minification"])
def test_gradients_are_bitwise_reproducible(name):
    a, b = _run(name), _run(name)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[3], b[3])
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))
    # through autograd: only the faces, only the flow
    f_only, c_only = _run(name, True, False), _run(name, False, True)
    assert f_only[3] is None and all(torch.equal(x, y) for x, y in zip(a[2], f_only[2]))
    assert all(g is None for g in c_only[2]) and torch.equal(a[3], c_only[3])


def test_each_gradient_alone_through_the_c_entry():
    """Any of the eight face-gradient pointers and grad_ctrl may be NULL: what is asked for alone is what the full call gives."""
    name = "all_faces"
    c = FC.make_case(name)
    _, idx, g_faces, g_ctrl = _run(name)
    faces, ctrl, cot = [f.to(DEV) for f in c["faces"]], c["ctrl"].to(DEV), c["cot"].to(DEV)
    (h, w), (Hf, Wf), (Hc, Wc) = ctrl.shape[:2], c["flow_hw"], c["crop_hw"]
    Cn, H, W = faces[0].shape
    fs = L.BagsFaces(len(faces), Cn, H, W)
    for i, t in enumerate(faces):
        fs.image[i] = t.data_ptr()
        for k in range(9):
            fs.mats[i][k] = float(c["mats"][i].reshape(-1)[k])
    ws = L.workspace(L.load().bags_resample_faces_workspace_size(len(faces), H, W, Hc, Wc), DEV)
    for want in list(range(len(faces))) + ["ctrl"]:
        outs = [torch.full_like(t, float("nan")) if want == i else None for i, t in enumerate(faces)]
        gc = torch.full_like(ctrl, float("nan")) if want == "ctrl" else None
        L.call("bags_resample_faces_backward", ctrl.device, fs, ctrl.data_ptr(), h, w, Hf, Wf, Hc, Wc, idx.data_ptr(), cot.data_ptr(), ws.data_ptr(),
               ws.numel(), L.ptr_table(outs + [None] * (L.MAX_FACES - len(outs))), L.ptr(gc))
        torch.cuda.synchronize()
        if want == "ctrl":
            assert torch.equal(gc, g_ctrl)
        else:
            assert torch.equal(outs[want], g_faces[want]), want


def test_one_face_and_the_identity_is_resample_image():
    g = torch.Generator().manual_seed(5)
    img = torch.rand(3, 33, 47, generator=g).to(DEV)
    gy, gx = torch.meshgrid(torch.linspace(-1.3, 1.3, 5), torch.linspace(-1.3, 1.3, 6), indexing="ij")
    ctrl = (torch.stack((gx, gy), -1) + 0.1 * torch.randn(5, 6, 2, generator=g)).to(DEV)
    out, idx = resample_faces([img], ctrl, torch.eye(3).unsqueeze(0), (40, 52), (31, 45))
    want, _ = resample_image(img, ctrl, (40, 52), (31, 45))
    inside = idx == 0
    assert 0.2 < float(inside.float().mean()) < 0.95 and bool(((idx == 0) | (idx == -1)).all())
    assert torch.equal(out[:, inside], want[:, inside]) and not bool(out[:, ~inside].any())


def test_cpu_tensors_raise():
    c = FC.make_case("all_faces")
    with pytest.raises(RuntimeError, match="GPU tensor"):
        resample_faces(c["faces"], c["ctrl"], c["mats"], c["flow_hw"], c["crop_hw"])
    with pytest.raises(RuntimeError, match="GPU tensor"):
        resample_faces([f.to(DEV) for f in c["faces"]], c["ctrl"], c["mats"], c["flow_hw"], c["crop_hw"])
    with pytest.raises(RuntimeError, match="exceeds"):
        resample_faces([f.to(DEV) for f in c["faces"]], c["ctrl"].to(DEV), c["mats"], c["flow_hw"], (c["flow_hw"][0] + 1, 8))
