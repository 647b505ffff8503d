"""The pieces of the path that CAN be pinned against the reference: SH basis, projection matrix, quaternion map,
photometric loss.  Golden vectors were produced by tests/golden/make_golden.py from /root/reference."""
import os

import numpy as np
import torch

from bags_raster import camera as cam
from bags_raster import loss as L
from oracle import raster_oracle as O


def test_sh_basis_matches_reference_eval_sh(golden_dir):
    g = np.load(os.path.join(golden_dir, "sh_basis.npz"))
    sh = torch.from_numpy(g["sh"])              # (64,3,16) channel-major as the reference's eval_sh takes it
    d = torch.from_numpy(g["dirs"])
    shs = sh.permute(0, 2, 1).contiguous()      # the op's (P,M,3) layout (scene/gaussian_model.py:131-134)
    for deg in range(4):
        got = O.eval_sh_rgb(deg, shs, d)
        np.testing.assert_allclose(got.numpy(), g[f"rgb_deg{deg}"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose((torch.from_numpy(g["rgb_in"]) - 0.5) / O.SH_C0, g["rgb2sh"], rtol=1e-6)


def test_projection_matrix_values_and_fov_jacobian(golden_dir):
    g = np.load(os.path.join(golden_dir, "camera_chain.npz"))
    for i, (fx, fy) in enumerate(g["fovs"]):
        fx_t, fy_t = torch.tensor(float(fx)), torch.tensor(float(fy))
        P = cam.projection_matrix(0.01, 100.0, fx_t, fy_t)
        np.testing.assert_allclose(P.numpy(), g["P"][i], rtol=1e-6, atol=1e-7)
        jx = torch.autograd.functional.jacobian(lambda a: cam.projection_matrix(0.01, 100.0, a, fy_t), fx_t)
        jy = torch.autograd.functional.jacobian(lambda a: cam.projection_matrix(0.01, 100.0, fx_t, a), fy_t)
        np.testing.assert_allclose(jx.numpy(), g["dP_dfovx"][i], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(jy.numpy(), g["dP_dfovy"][i], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(cam.projection_matrix(0.01, 100.0, 0.6911112, 1.0).numpy(), g["P_float"], rtol=1e-6)


def test_quaternion_to_rotation_values_and_jacobian(golden_dir):
    g = np.load(os.path.join(golden_dir, "camera_chain.npz"))
    for q, R, J in zip(g["q"], g["R"], g["dR_dq"]):
        qt = torch.from_numpy(q)
        np.testing.assert_allclose(cam.quaternion_to_rotation(qt).numpy(), R, rtol=1e-5, atol=1e-6)
        Jg = torch.autograd.functional.jacobian(cam.quaternion_to_rotation, qt)
        np.testing.assert_allclose(Jg.numpy(), J, rtol=1e-4, atol=1e-5)
        # round trip through the inverse map used for init_quaternion (scene/cameras.py:98)
        R_t = torch.from_numpy(R)
        q2 = cam.rotation_to_quaternion(R_t)
        np.testing.assert_allclose(cam.quaternion_to_rotation(q2).numpy(), R, rtol=1e-4, atol=1e-5)


def test_photometric_loss_matches_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "loss.npz"))
    a = torch.from_numpy(g["a"]).requires_grad_(True)
    b = torch.from_numpy(g["b"])
    assert abs(L.l1_loss(a, b).item() - float(g["l1"])) < 1e-6
    assert abs(L.ssim(a, b).item() - float(g["ssim"])) < 1e-5
    loss = L.photometric_loss(a, b)
    assert abs(loss.item() - float(g["loss"])) < 1e-5
    (ga,) = torch.autograd.grad(loss, a)
    np.testing.assert_allclose(ga.numpy(), g["dloss_da"], rtol=1e-3, atol=1e-7)


def test_pose_camera_chain_consistency():
    """viewmatrix = W2C^T, projmatrix = viewmatrix @ intrinsic, campos = inverse(viewmatrix)[3,:3]
    (scene/cameras.py:105-113,359-381) and gradients reach the four pose leaves."""
    R = cam.quaternion_to_rotation(torch.tensor([0.9, 0.1, -0.2, 0.3]))
    T = torch.tensor([0.2, -0.1, 4.0])
    c = cam.PoseCamera(R, T, 1.1, 0.7, 64, 48)
    V = c.get_world_view_transform()
    w2c = torch.eye(4); w2c[:3, :3] = R.t(); w2c[:3, 3] = T
    np.testing.assert_allclose(V.detach().numpy(), w2c.t().numpy(), atol=1e-6)
    np.testing.assert_allclose(c.get_full_proj_transform().detach().numpy(), (V @ c.get_intrinsic()).detach().numpy(), atol=1e-6)
    np.testing.assert_allclose(c.get_camera_center().detach().numpy(), (-R @ T).numpy(), atol=1e-5)
    s = c.get_full_proj_transform().sum() + c.get_camera_center().sum()
    grads = torch.autograd.grad(s, c.pose_leaves())
    assert all(torch.isfinite(g).all() and g.abs().sum() > 0 for g in grads)


def test_product_eval_sh_matches_reference(golden_dir):
    """bags_raster.gaussians.eval_sh is the colour path render() takes for hybrid / convert_SHs_python
    (gaussian_renderer/__init__.py:90-95): same (…, C, K) layout as utils/sh_utils.py:57."""
    from bags_raster import gaussians as G
    g = np.load(os.path.join(golden_dir, "sh_basis.npz"))
    sh, d = torch.from_numpy(g["sh"]), torch.from_numpy(g["dirs"])
    for deg in range(4):
        np.testing.assert_allclose(G.eval_sh(deg, sh, d).numpy(), g[f"rgb_deg{deg}"], rtol=1e-5, atol=1e-6)
    rgb = torch.from_numpy(g["rgb_in"])
    np.testing.assert_allclose(G.RGB2SH(rgb).numpy(), g["rgb2sh"], rtol=1e-6)
    np.testing.assert_allclose(G.SH2RGB(G.RGB2SH(rgb)).numpy(), g["sh2rgb"], rtol=1e-6)


def test_gaussian_activations_match_reference(golden_dir):
    """build_rotation / build_scaling_rotation / strip_lowerdiag / covariance activation / quaternion_multiply /
    inverse_sigmoid against the reference's own functions (utils/general_utils.py:114-163,
    scene/gaussian_model.py:27-31, gaussian_renderer/__init__.py:19-28)."""
    from bags_raster import gaussians as G
    from bags_raster.render import quaternion_multiply
    g = np.load(os.path.join(golden_dir, "gaussian_activations.npz"))
    s, r = torch.from_numpy(g["scaling"]), torch.from_numpy(g["rotation"])
    # R's entries are 1 - 2 (y^2 + z^2) and the like: an entry near 0 carries the rounding of operands near 1, so the bound is a few
    # float32 ulps of 1.0 (torch on another host rounds the same float32 formula up to 3 ulps apart); relative 1e-6 as before
    ulp1 = float(np.finfo(np.float32).eps)
    np.testing.assert_allclose(G.build_rotation(r).numpy(), g["R"], rtol=1e-6, atol=4 * ulp1)
    np.testing.assert_allclose(G.build_scaling_rotation(s, r).numpy(), g["L"], rtol=1e-6, atol=4 * ulp1 * float(s.abs().max()))
    np.testing.assert_allclose(G.covariance_from_scaling_rotation(s, 1.0, r).numpy(), g["cov_mod1"], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(G.covariance_from_scaling_rotation(s, 0.7, r).numpy(), g["cov_mod07"], rtol=1e-5, atol=1e-7)
    sg, rg = s.clone().requires_grad_(True), r.clone().requires_grad_(True)
    (G.covariance_from_scaling_rotation(sg, 0.7, rg) * torch.from_numpy(g["cov_weights"])).sum().backward()
    np.testing.assert_allclose(sg.grad.numpy(), g["dcov_dscaling"], rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(rg.grad.numpy(), g["dcov_drotation"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(quaternion_multiply(torch.from_numpy(g["qa"]), torch.from_numpy(g["qb"])).numpy(), g["qa_qb"],
                               rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(G.inverse_sigmoid(torch.from_numpy(g["p"])).numpy(), g["inverse_sigmoid_p"], rtol=1e-6)


def test_gaussian_bag_round_trips_activations():
    """from_activated inverts exp / sigmoid / keeps unit quaternions: the activated values come back, get_features has the
    (P,K,3) layout the op takes, and the densification accumulators consume .grad[:, :2] norms
    (scene/gaussian_model.py:449-455)."""
    from bags_raster import gaussians as G
    from bags_raster.synth import synth_scene
    sc = synth_scene(50, 3, 0.5, 3)
    pc = G.GaussianBag.from_activated(sc, 3)
    assert pc.active_sh_degree == 3 and pc.max_sh_degree == 3
    np.testing.assert_allclose(pc.get_scaling.detach().numpy(), sc["scales"].numpy(), rtol=1e-6)
    np.testing.assert_allclose(pc.get_opacity.detach().numpy(), sc["opacities"].numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(pc.get_rotation.detach().numpy(), sc["rotations"].numpy(), rtol=1e-6, atol=1e-7)
    assert pc.get_features.shape == (50, 16, 3) and torch.equal(pc.get_features.detach(), sc["shs"])
    cov = pc.get_covariance(1.0)
    L = G.build_scaling_rotation(sc["scales"], sc["rotations"])
    np.testing.assert_allclose(cov.detach().numpy(), G.strip_symmetric(L @ L.transpose(1, 2)).numpy(), rtol=1e-5, atol=1e-9)
    vp = torch.zeros(50, 3, requires_grad=True); vpd = torch.zeros(50, 3, requires_grad=True)
    vp.grad = torch.ones(50, 3) * 3.0; vpd.grad = torch.ones(50, 3) * 4.0
    flt = torch.arange(50) % 2 == 0
    pc.add_densification_stats(vp, vpd, flt, abs_grad=False)
    pc.add_densification_stats(vp, vpd, flt, abs_grad=True)
    want = (3.0 + 4.0) * (2.0 ** 0.5)
    assert torch.allclose(pc.xyz_gradient_accum[flt], torch.full((25, 1), want)) and (pc.xyz_gradient_accum[~flt] == 0).all()
    assert (pc.denom[flt] == 2).all()


def test_loss_oracle_matches_reference(golden_dir):
    """oracle/loss_oracle.py (numpy, dense 121-tap window, analytic adjoint) against the reference's l1_loss / ssim values
    and autograd gradients (utils/loss_utils.py:18-19,48-76)."""
    from oracle import loss_oracle as LO
    g = np.load(os.path.join(golden_dir, "loss.npz"))
    l1, s, grad = LO.loss_and_grad(g["a"], g["b"], 0.8, -0.2)          # d/da of 0.8 L1 + 0.2 (1 - SSIM)
    assert abs(l1 - float(g["l1"])) < 1e-6 and abs(s - float(g["ssim"])) < 1e-5
    assert abs(0.8 * l1 + 0.2 * (1 - s) - float(g["loss"])) < 1e-5
    np.testing.assert_allclose(grad, g["dloss_da"], rtol=1e-3, atol=2e-8)
    g = np.load(os.path.join(golden_dir, "loss_odd.npz"))
    l1, s, g1 = LO.loss_and_grad(g["a"], g["b"], 1.0, 0.0)
    _, _, g2 = LO.loss_and_grad(g["a"], g["b"], 0.0, 1.0)
    assert abs(l1 - float(g["l1"])) < 1e-6 and abs(s - float(g["ssim"])) < 1e-5
    np.testing.assert_allclose(g1, g["dl1_da"], rtol=1e-6, atol=1e-10)
    np.testing.assert_allclose(g2, g["dssim_da"], rtol=2e-3, atol=3e-8)
    np.testing.assert_allclose(LO.window_2d().sum(), 1.0, rtol=1e-6)


def test_resample_oracle_and_torch_pipeline_match_reference(golden_dir):
    """oracle/resample_oracle.py (numpy, explicit taps and adjoint) and bags_raster.distortion.resample_image_torch against the
    reference's own apply_distortion / center_crop (utils/util_distortion.py:58-77,271-311).  The reference crops with a
    second grid_sample whose integer grid is only reproduced to ~1e-4 px, hence the 2e-4 absolute bar."""
    from oracle import resample_oracle as RO
    from bags_raster.distortion import resample_image_torch
    g = np.load(os.path.join(golden_dir, "resample.npz"))
    fhw, chw = tuple(int(v) for v in g["flow_hw"]), tuple(int(v) for v in g["crop_hw"])
    out, mask = RO.forward(g["image"], g["ctrl"], fhw, chw)
    np.testing.assert_allclose(out, g["out"], atol=2e-4)
    assert (mask != g["mask"]).mean() < 0.002                          # pixels that are exactly 0 in one and 1e-7 in the other
    gi, gc = RO.backward(g["image"], g["ctrl"], fhw, chw, g["cot"])
    np.testing.assert_allclose(gi, g["d_image"], atol=3e-4)
    np.testing.assert_allclose(gc, g["d_ctrl"], rtol=2e-3, atol=2e-3 * np.abs(g["d_ctrl"]).max())
    img = torch.from_numpy(g["image"]).requires_grad_(True); ctl = torch.from_numpy(g["ctrl"]).requires_grad_(True)
    o2, m2 = resample_image_torch(img, ctl, fhw, chw)
    np.testing.assert_allclose(o2.detach().numpy(), g["out"], atol=1e-6)
    assert np.array_equal(m2.numpy(), g["mask"])
    (o2 * torch.from_numpy(g["cot"])).sum().backward()
    np.testing.assert_allclose(img.grad.numpy(), g["d_image"], atol=1e-6)
    np.testing.assert_allclose(ctl.grad.numpy(), g["d_ctrl"], rtol=1e-4, atol=1e-4)


def test_resample_oracle_flow_matches_interpolate(golden_dir):
    """RO.interpolated_flow (what bags_resample_forward's flow_out is held to) against F.interpolate(bilinear,
    align_corners=False) in float64 followed by the integer crop, on the golden geometry."""
    import torch.nn.functional as F
    from oracle import resample_oracle as RO
    g = np.load(os.path.join(golden_dir, "resample.npz"))
    fhw, chw = tuple(int(v) for v in g["flow_hw"]), tuple(int(v) for v in g["crop_hw"])
    flow = RO.interpolated_flow(g["ctrl"], fhw, chw)
    assert flow.shape == chw + (2,) and flow.dtype == np.float64
    up = F.interpolate(torch.from_numpy(g["ctrl"]).double().permute(2, 0, 1).unsqueeze(0), size=fhw, mode="bilinear",
                       align_corners=False)[0].permute(1, 2, 0).numpy()
    y0, x0 = (fhw[0] - chw[0]) // 2, (fhw[1] - chw[1]) // 2
    np.testing.assert_allclose(flow, up[y0:y0 + chw[0], x0:x0 + chw[1]], rtol=0, atol=1e-12)


def test_loss_cases_and_float32_error_cpu():
    """The CPU half of tests/test_loss_gpu.py's measured bar (tests/loss_cases.py): every input class is what it says, and the
    float32 PyTorch loss is within 1e-6 (relative, gradient) of the float64 oracle except on the flat bright image, where
    E[a^2] - mu^2 cancels against C2 = 9e-4."""
    import loss_cases as LC
    for shape in LC.RAGGED_SHAPES:
        assert shape[2] % 4 == 0 and shape[2] % 32 != 0
        for kind in LC.KINDS:
            a, b = LC.make_pair(kind, shape)
            a2, b2 = LC.make_pair(kind, shape)
            assert a.shape == shape and a.dtype == np.float32 and b.dtype == np.float32 and a.flags.c_contiguous
            assert np.array_equal(a, a2) and np.array_equal(b, b2)
            if kind == "noise":
                assert np.array_equal(a[..., : shape[2] // 2], b[..., : shape[2] // 2]) and 0 <= a.min() and a.max() < 1
            elif kind == "flat_bright":
                assert abs(a.mean() - 0.9) < 1e-3 and np.abs(a - 0.9).max() < 6e-3 and np.abs(b - 0.9).max() < 6e-3
            elif kind == "dark":
                assert 0 <= min(a.min(), b.min()) and max(a.max(), b.max()) < 1e-3
            elif kind == "out_of_range":
                assert -1 <= a.min() and a.max() < 2 and 0 <= b.min() and b.max() < 1
                assert shape[1] * shape[2] < 100 or (a.min() < 0 and a.max() > 1)
            else:
                assert set(np.unique(a)) <= {0.0, 1.0} and np.array_equal(a[..., 1:], b[..., :-1])
                assert np.array_equal(a[:, : max(shape[1] - 7, 0)], 1 - a[:, 7:]) and np.array_equal(a[..., : max(shape[2] - 5, 0)], 1 - a[..., 5:])
            r = LC.reference(a, b)
            if r["scale"] == 0.0:                        # the (2,5,4) checkerboard is one cell: both images zero, no gradient
                assert kind == "checkerboard" and shape == (2, 5, 4) and r["err32_grad"] == 0.0
            rel = r["err32_grad"] / max(r["scale"], 1e-300)
            print(f"{kind:13s} {shape}: err32 grad {rel:.2e} rel, l1 {r['err32_l1']:.1e}, ssim {r['err32_ssim']:.1e}")
            assert np.isfinite(r["grad"]).all()
            assert rel < (1e-3 if kind == "flat_bright" else 1e-6), (kind, shape, rel)
            assert r["err32_l1"] < 1e-6 and r["err32_ssim"] < 1e-5


def _pose_camera_from_golden(g, i, device="cpu"):
    from bags_raster.camera import PoseCamera
    c = PoseCamera(torch.eye(3), torch.zeros(3), 1.0, 1.0, 64, 48, device=device)
    x = torch.tensor(g["x"][i])
    with torch.no_grad():
        c.init_quaternion.copy_(torch.tensor(g["init_quaternion"][i]))
        c.init_translation.copy_(torch.tensor(g["init_translation"][i]))
    return c, x


def test_composed_pose_chain_matches_reference_methods(golden_dir):
    """scene/cameras.py:356-381 as the reference's own METHODS compute it (camera_pose_chain.npz: bodies of
    Camera.get_world_view_transform / get_full_proj_transform / get_camera_center / get_intrinsic run on a stub self), with and
    without global alignment: values of the four tensors the op consumes and their Jacobians with respect to
    delta_quaternion, delta_translation, learnable_fovx / fovy, the global rotation and the translation scale."""
    g = np.load(os.path.join(golden_dir, "camera_pose_chain.npz"))
    for i in range(g["x"].shape[0]):
        c, x = _pose_camera_from_golden(g, i)

        def run(v):
            from bags_raster import camera as cam        # functional evaluation of the same chain on one packed vector
            q = c.init_quaternion + v[0:4]
            rot = v[9:18].view(3, 3) @ cam.quaternion_to_rotation(q)
            t = c.init_translation + v[4:7].view(3, 1)
            w2c_t = torch.cat((torch.cat((rot, t), dim=1), c.last_row), dim=0).t()
            c2w = w2c_t.inverse()
            mask = torch.ones_like(c2w).index_put((torch.tensor([3, 3, 3]), torch.tensor([0, 1, 2])), v[18:19].expand(3))
            V = (c2w * mask).inverse()
            K = cam.projection_matrix(c.znear, c.zfar, v[7], v[8]).transpose(0, 1)
            return torch.cat([V.reshape(-1), (V @ K).reshape(-1), K.reshape(-1), V.inverse()[3, :3]])
        # 1. the module's own getters (what bench / tests / render() call) reproduce the reference values
        with torch.no_grad():
            c.delta_quaternion.copy_(x[0:4]); c.delta_translation.copy_(x[4:7].view(3, 1))
            c.learnable_fovx.copy_(x[7]); c.learnable_fovy.copy_(x[8])
        G, sc = x[9:18].view(3, 3), x[18:19]
        got = torch.cat([c.get_world_view_transform(G, sc).reshape(-1), c.get_full_proj_transform(G, sc).reshape(-1),
                         c.get_intrinsic().reshape(-1), c.get_camera_center(G, sc)]).detach()
        assert np.allclose(got.numpy(), g["y"][i], rtol=2e-5, atol=2e-6), np.abs(got.numpy() - g["y"][i]).max()
        if i < 2:                                             # identity alignment == the getters called without arguments
            got0 = torch.cat([c.get_world_view_transform().reshape(-1), c.get_full_proj_transform().reshape(-1),
                              c.get_intrinsic().reshape(-1), c.get_camera_center()]).detach()
            assert np.allclose(got0.numpy(), g["y"][i], rtol=2e-5, atol=2e-6)
        # 2. Jacobians: autograd through the getters (leaves + alignment) against the reference's autograd
        leaves = c.pose_leaves()
        Gr, sr = G.clone().requires_grad_(True), sc.clone().requires_grad_(True)
        y = torch.cat([c.get_world_view_transform(Gr, sr).reshape(-1), c.get_full_proj_transform(Gr, sr).reshape(-1),
                       c.get_intrinsic().reshape(-1), c.get_camera_center(Gr, sr)])
        J = g["dy_dx"][i]
        rows = np.random.RandomState(i).choice(51, 12, replace=False)
        for r in rows:
            gs = torch.autograd.grad(y[r], leaves + [Gr, sr], retain_graph=True, allow_unused=True)
            flat = torch.cat([torch.zeros_like(t).reshape(-1) if a is None else a.reshape(-1) for a, t in zip(gs, leaves + [Gr, sr])])
            assert np.allclose(flat.numpy(), J[r], rtol=2e-4, atol=2e-5), (r, np.abs(flat.numpy() - J[r]).max())
        # 3. the functional restatement above (used nowhere else) agrees too: guards the test's own plumbing
        assert np.allclose(run(x).detach().numpy(), g["y"][i], rtol=2e-5, atol=2e-6)
