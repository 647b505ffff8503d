"""GPU checks of the opt-in depth / weights gradients (GaussianRasterizationSettings.depth_weights_grad, ABI 11): every gradient
tensor against the two-call reference of tests/depth_oracle.py (fp32 walk and fp64 replay), the default path unchanged, the
extras through every backward mode, and a pose pulled back by a depth loss alone."""
import math

import pytest
import torch

from depth_oracle import compare_ex, cotangents, path_scene, run_hip_ex
from parity import sample_tiles
from scenes import make_case

pytestmark = pytest.mark.gpu


def _assert_ex(rep, grad_tol=1e-4, shift_tol=1e-3):
    """Best of (fp32 reference, fp64 replay) within grad_tol for every tensor; shift_factors (an identically zero parameter whose
    gradient is a near-cancelling sum, see test_parity_gpu.py) within shift_tol.  Never further from fp64 than the fp32
    reference itself is (x1.5 slack)."""
    print(rep)
    g32, g64 = rep["grad_rel_fp32"], rep.get("grad_rel_fp64", rep["grad_rel_fp32"])
    assert g32, rep
    for k, e in g32.items():
        best = min(e, g64.get(k, e))
        assert best <= (shift_tol if k == "shift_factors" else grad_tol), (k, best, rep)
        if "oracle32_vs_64" in rep and k != "shift_factors":
            assert g64[k] <= 1.5 * rep["oracle32_vs_64"][k] + 1e-5, (k, g64[k], rep["oracle32_vs_64"][k])


CASES = {
    "sh3": dict(),
    "colors_cov3D": dict(precomp=True),
    "shift": dict(shift=torch.tensor([0.02, -0.01, 0.005])),
    "depth_key_distance": dict(depth_key="distance"),
    "aabb": dict(tile_bounds="aabb"),
    "radix": dict(binning="radix"),
    "frozen_camera": dict(frozen_camera=True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_depth_weights_gradients_match_reference(case):
    scene, cam = make_case(1500, 128, 96, 1.0, 3, seed=11)
    kw = dict(CASES[case])
    if kw.pop("precomp", False):
        g = torch.Generator().manual_seed(3)
        kw["colors"] = torch.rand(1500, 3, generator=g)
        s, q = scene["scales"], torch.nn.functional.normalize(scene["rotations"], dim=1)
        w, x, y, z = q.unbind(1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                         2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                         2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
        L = R * s[:, None, :]
        S = L @ L.transpose(1, 2)
        kw["cov3D"] = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).contiguous()
    _assert_ex(compare_ex(scene, cam, 3, seed=4, **kw))


@pytest.mark.parametrize("which", ["depth", "weights"])
def test_loss_from_one_extra_output_alone(which):
    """grad_color is None (the image is not in the loss): NULL to the library, the EXTRA kernels read it as zero."""
    scene, cam = make_case(1500, 128, 96, 1.0, 3, seed=12)
    _assert_ex(compare_ex(scene, cam, 3, seed=5, image=False, depth=which == "depth", weights=which == "weights"))


def test_forced_dense_mode_with_extras():
    """The dense-scene mode (a byte per record instead of zero records) with the extras: same bits as the default mode, and
    the reference's gradients."""
    from bags_raster import rasterizer as R
    scene, cam = make_case(1500, 128, 96, 1.0, 3, seed=13)
    gi, gd, gw = cotangents(96, 128, 6)
    _, a = run_hip_ex(scene, cam, 3, gi, gd, gw)
    old = R.DENSE_PER_TILE
    try:
        R.DENSE_PER_TILE = 1
        _, b = run_hip_ex(scene, cam, 3, gi, gd, gw)
        _assert_ex(compare_ex(scene, cam, 3, seed=6))
    finally:
        R.DENSE_PER_TILE = old
    for k, v in a.items():
        assert (v is None) == (b[k] is None) and (v is None or torch.equal(v, b[k])), k


@pytest.mark.timeout(900)
def test_full_size_config3_sampled_tiles():
    """BASELINE config 3 (500 k Gaussians, 1080p, SH 3, pose gradients) with all three cotangents confined to 96 sampled tiles
    (as test_full_size_config3_aabb: zero cotangents contribute exact zeros, so every gradient tensor stays comparable)."""
    import os
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    W, H = 1920, 1080
    scene, cam = make_case(500_000, W, H, 0.5, 3, seed=0)
    rep = compare_ex(scene, cam, 3, seed=2, tiles=sample_tiles(W, H, 96, seed=3), check_fp64=True)
    _assert_ex(rep)


def _grads(scene, cam, gi, gd, gw, keyword=True):
    return run_hip_ex(scene, cam, 3, gi, gd, gw, depth_weights_grad=keyword)[1]


def _equal(a, b):
    for k in a:
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert torch.equal(a[k], b[k]), (k, (a[k] - b[k]).abs().max().item())


def test_keyword_on_with_image_loss_only_is_the_default_path():
    """depth / weights not in the loss: their cotangents are None, the library gets no extras and runs the default kernels --
    every gradient torch.equal to the keyword off."""
    scene, cam = make_case(1500, 128, 96, 1.0, 3, seed=14)
    gi, _, _ = cotangents(96, 128, 7)
    _equal(_grads(scene, cam, gi, None, None, True), _grads(scene, cam, gi, None, None, False))


def test_zero_extra_cotangents_leave_the_image_gradients():
    """depth and weights in the graph with zero cotangents: the EXTRA kernels run and add exact zeros to every (pixel, splat)
    term.  Their wave copies of the sums hold 16 fewer slots, so a chunk in which more than SL - 16 staged splats reach one
    quadrant is processed in two halves and its scan is grouped differently: hence 1e-6 relative, not torch.equal."""
    from scenes import rel_err
    scene, cam = make_case(1500, 128, 96, 1.0, 3, seed=14)
    gi, gd, gw = cotangents(96, 128, 7)
    a = _grads(scene, cam, gi, None, None, False)
    b = _grads(scene, cam, gi, torch.zeros_like(gd), torch.zeros_like(gw), True)
    for k in a:
        if a[k] is not None:
            assert rel_err(b[k], a[k]) <= 1e-6, k
    # a depth cotangent that is not zero moves them (the test above is not vacuous)
    c = _grads(scene, cam, gi, gd, None, True)
    assert rel_err(c["means3D"], a["means3D"]) > 1e-3 and rel_err(c["viewmatrix"], a["viewmatrix"]) > 1e-4


def test_extras_are_bitwise_reproducible():
    scene, cam = make_case(3000, 160, 128, 1.0, 3, seed=15)
    gi, gd, gw = cotangents(128, 160, 8)
    _equal(_grads(scene, cam, gi, gd, gw), _grads(scene, cam, gi, gd, gw))


def test_extras_with_the_split_and_accumulating_backwards():
    """AccumulationGate (phase BLEND, then PREPROCESS: both calls get the extras), ACCUMULATE_IN_PLACE and FactoredSH with the
    depth / weights cotangents give what one plain call gives."""
    from bags_raster import GaussianRasterizer
    from bags_raster import rasterizer as R
    from scenes import camera_tensors, hip_settings
    dev = torch.device("cuda")
    scene, cam = make_case(1500, 128, 96, 1.0, 3, seed=16)
    gi, gd, gw = [x.to(dev) for x in cotangents(96, 128, 9)]

    def run(mode):
        t = {k: v.to(dev).clone().requires_grad_(True) for k, v in scene.items()}
        ct = {k: v.clone().requires_grad_(True) for k, v in camera_tensors(cam, dev).items()}
        P = t["means3D"].shape[0]
        st = hip_settings(cam, 3, dev, tensors=ct)._replace(depth_weights_grad=True)
        if mode == "in_place":
            for v in t.values():
                v.grad = torch.zeros_like(v)
        old = (R.ACCUMULATION_GATE, R.ACCUMULATE_IN_PLACE, R.FACTORED_SH)
        try:
            R.ACCUMULATION_GATE = R.AccumulationGate() if mode == "gate" else None
            R.ACCUMULATE_IN_PLACE = mode == "in_place"
            R.FACTORED_SH = R.FactoredSH() if mode == "factored" else None
            fsh = R.FACTORED_SH
            img, _, depth, weights, _ = GaussianRasterizer(st)(
                means3D=t["means3D"], means2D=torch.zeros(P, 3, device=dev, requires_grad=True),
                means2D_densify=torch.zeros(P, 3, device=dev, requires_grad=True), shift_factors=torch.zeros(3, device=dev, requires_grad=True),
                shs=t["shs"], colors_precomp=None, opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"], cov3D_precomp=None)
            torch.autograd.backward([img, depth, weights], [gi, gd, gw])
            if fsh is not None:
                fsh.finish(t["means3D"], t["shs"])
        finally:
            R.ACCUMULATION_GATE, R.ACCUMULATE_IN_PLACE, R.FACTORED_SH = old
        return {k: v.grad.detach().cpu() for k, v in {**t, **ct}.items()}

    ref = run("plain")
    for mode in ("gate", "in_place", "factored"):
        _equal(run(mode), ref)


# ---- every path of the EXTRA backward against the oracle.  tests/test_depth_grad_cpu.py proves from the oracle alone that each scene
# takes the path it is named for (chunk geometry, dense-scene mode, chunks that only the extras split, ...).
def _report(name, rep):
    from parity import dump_report
    dump_report(name, rep)


def _path_case(name, tile_bounds, depth_only=False, **kw):
    scene, cam, deg = path_scene(name, tile_bounds)
    res = compare_ex(scene, cam, deg, seed=21, tile_bounds=tile_bounds, image=not depth_only, weights=not depth_only, **kw)
    _report(f"extras_{name}[{tile_bounds}{',depth_only' if depth_only else ''}]", res[0] if kw.get("return_oracle") else res)
    return res


@pytest.mark.parametrize("cotangents_on", ["all", "depth_only"])
@pytest.mark.parametrize("tile_bounds", ["opacity", "aabb"])
@pytest.mark.parametrize("name", ["band_sparse", "band_dense", "overflow"])
def test_extras_on_split_chunks(name, tile_bounds, cotangents_on):
    """band_*: chunks whose fullest quadrant lies between SL - 16 and SL run in one pass in the default kernel and in two halves here (the
    one branch the extras add to the control flow), in both chunk geometries (240 / 168 and 224 / 176) and from consecutive and from
    compacted lists; overflow: every full chunk in two halves.  With the depth cotangent alone dL/dz (the twelfth sum of a slot)
    carries the whole gradient."""
    _assert_ex(_path_case(name, tile_bounds, cotangents_on == "depth_only"))


def test_extras_in_the_dense_scene_mode(monkeypatch):
    """525 instances per tile: the library's own threshold picks the dense-scene mode (live bytes; preprocess_bwd must not read the
    dL/dz of a record nobody wrote).  The oracle's bars, and bit for bit what the zero-record mode gives."""
    from bags_raster import rasterizer as R
    scene, cam, deg = path_scene("dense_mode")
    gi, gd, gw = cotangents(48, 64, 21)
    monkeypatch.setattr(R, "DENSE_PER_TILE", 0)
    _assert_ex(_path_case("dense_mode", "opacity"))
    _, a = run_hip_ex(scene, cam, deg, gi, gd, gw)
    monkeypatch.setattr(R, "DENSE_PER_TILE", -1)
    _, b = run_hip_ex(scene, cam, deg, gi, gd, gw)
    _equal(a, b)


def test_extras_on_saturated_pixels():
    """Opaque splats: every pixel stops at T < 1e-4 long before its list ends -- dL/dweights and dL/ddepth of the splats behind the cut
    are exactly absent in the reference (they are not in its graph)."""
    rep, o = _path_case("saturated", "opacity", return_oracle=True)
    _assert_ex(rep)
    lens = (o["ranges"][:, 1] - o["ranges"][:, 0]).reshape(6, 6)            # 96 x 96: 6 x 6 tiles
    assert (o["n_contrib"] < lens.repeat(16, 0).repeat(16, 1)).mean() > 0.5  # the walk this run was compared on did end early


@pytest.mark.parametrize("W,H", [(100, 70), (17, 33)])
def test_extras_on_tiles_that_overhang_the_image(W, H):
    scene, cam = make_case(800, W, H, 2.0, 2, seed=W)
    rep = compare_ex(scene, cam, 2, seed=22)
    _report(f"extras_ragged[{W}x{H}]", rep)
    _assert_ex(rep)


@pytest.mark.parametrize("case", ["tiny_scales", "huge_scales", "opaque_and_transparent", "near_plane", "off_screen", "needle"])
def test_extras_on_extreme_inputs(case):
    """The six inputs of test_extreme_inputs_match_oracle with all three cotangents, to that test's bars."""
    scene, cam = make_case(600, 144, 112, 2.0, 1, seed=41)
    g = torch.Generator().manual_seed(43)
    if case == "tiny_scales":
        scene["scales"] = scene["scales"] * 1e-4
    elif case == "huge_scales":
        scene["scales"] = scene["scales"] * 40.0
        scene["opacities"] = scene["opacities"] * 0.3
    elif case == "opaque_and_transparent":
        op = torch.rand(600, 1, generator=g)
        scene["opacities"] = torch.where(op < 0.3, torch.zeros_like(op), torch.where(op > 0.7, torch.full_like(op, 0.9999), op))
    elif case == "near_plane":
        scene["means3D"] = scene["means3D"] * torch.tensor([1.0, 1.0, 0.05]) + torch.tensor([0.0, 0.0, -3.8])   # z_view ~ 0.2
    elif case == "off_screen":
        scene["means3D"] = scene["means3D"] + torch.tensor([2.6, -1.9, 0.0])
    elif case == "needle":
        scene["scales"] = scene["scales"] * torch.tensor([30.0, 0.02, 0.02])
    rep = compare_ex(scene, cam, 1, seed=23)
    _report(f"extras_extreme[{case}]", rep)
    if case == "needle":
        print(rep)
        # parity.assert_ill_conditioned's rule: fp32 itself is only good to ~1e-2 here; at most 3x as far from fp64 as the fp32 reference
        for k, ref in rep["oracle32_vs_64"].items():
            if k in rep["grad_rel_fp64"]:
                assert rep["grad_rel_fp64"][k] <= 3.0 * ref + 1e-4, (k, rep["grad_rel_fp64"][k], ref)
    else:
        _assert_ex(rep, grad_tol=3e-4)


@pytest.mark.parametrize("setting", ["scale_modifier", "clamp_exact", "conic_exact"])
def test_extras_with_other_settings(setting):
    if setting == "scale_modifier":
        scene, cam = make_case(1500, 96, 64, 2.0, 3, seed=3)
        rep = compare_ex(scene, cam, 3, seed=24, scale_modifier=0.7)
    elif setting == "clamp_exact":        # camera close to the cloud: Gaussians beyond 1.3 x the field of view reach the image
        scene, cam = make_case(1500, 96, 64, 2.0, 1, seed=3, dist=2.5)
        rep = compare_ex(scene, cam, 1, seed=24, clamp_grad="exact")
    else:                                 # small splats: det(cov2D) near its floor, where the stock regulariser weighs most
        scene, cam = make_case(2000, 96, 64, 0.25, 1, seed=9)
        rep = compare_ex(scene, cam, 1, seed=24, conic_grad="exact")
    _report(f"extras_settings[{setting}]", rep)
    _assert_ex(rep)


def test_extras_with_no_one_and_no_visible_gaussian():
    from bags_raster.synth import look_at_origin_camera
    cam = look_at_origin_camera(64, 48)
    gi, gd, gw = cotangents(48, 64, 25)
    # P = 0: no error, every gradient of its tensor's shape and zero
    empty = dict(means3D=torch.zeros(0, 3), scales=torch.zeros(0, 3), rotations=torch.zeros(0, 4), opacities=torch.zeros(0, 1),
                 shs=torch.zeros(0, 4, 3))
    outs, grads = run_hip_ex(empty, cam, 1, gi, gd, gw)
    assert float(outs[2].abs().max()) == 0.0 and float(outs[3].abs().max()) == 0.0
    for k, v in grads.items():
        assert v is None or float(v.abs().sum()) == 0.0, k
        if v is not None and k in empty:
            assert v.shape == empty[k].shape, k
    # everything behind the camera: no instance, zero gradients
    scene, _ = make_case(50, 64, 48, 1.0, 1, seed=1)
    scene["means3D"] = scene["means3D"] + torch.tensor([0.0, 0.0, -10.0])
    outs, grads = run_hip_ex(scene, cam, 1, gi, gd, gw)
    assert int(outs[1].max()) == 0 and float(outs[3].abs().max()) == 0.0
    assert all(v is None or float(v.abs().max()) == 0.0 for v in grads.values())
    # a single Gaussian on the optical axis
    one = dict(means3D=torch.zeros(1, 3), scales=torch.full((1, 3), 0.2), rotations=torch.tensor([[1.0, 0, 0, 0]]),
               opacities=torch.tensor([[0.8]]), shs=torch.randn(1, 16, 3, generator=torch.Generator().manual_seed(2)) * 0.3)
    rep = compare_ex(one, cam, 3, seed=25)
    _report("extras_single", rep)
    _assert_ex(rep)


def test_background_does_not_reach_the_extra_gradients():
    """depth and weights composite over background 0 whatever the image's background is: with the image out of the loss the
    gradients with bg = (0.3, 0.7, 0.1) are those with bg = 0, bit for bit (tile_begin forms bg . dL/dimage from zeros)."""
    scene, cam = make_case(1500, 96, 64, 2.0, 3, seed=3)
    _, gd, gw = cotangents(64, 96, 26)
    a = run_hip_ex(scene, cam, 3, None, gd, gw)[1]
    b = run_hip_ex(scene, cam, 3, None, gd, gw, bg=torch.tensor([0.3, 0.7, 0.1]))[1]
    assert float(a["means3D"].abs().sum()) > 0
    _equal(a, b)


def test_zero_extra_cotangents_on_a_band_scene():
    """test_zero_extra_cotangents_leave_the_image_gradients on band_sparse: 7 of its 18 chunks run in one pass in the default kernel and in
    two halves with the extras, so the image gradients agree to 1e-6 -- and NOT to the bit: the two-half branch, that test's reason for
    its bar, did run."""
    from scenes import rel_err
    scene, cam, deg = path_scene("band_sparse")
    gi, gd, gw = cotangents(48, 64, 27)
    a = run_hip_ex(scene, cam, deg, gi, None, None, depth_weights_grad=False)[1]
    b = run_hip_ex(scene, cam, deg, gi, torch.zeros_like(gd), torch.zeros_like(gw))[1]
    same = True
    for k in a:
        if a[k] is not None:
            assert rel_err(b[k], a[k]) <= 1e-6, (k, rel_err(b[k], a[k]))
            same = same and torch.equal(a[k], b[k])
    assert not same


def test_depth_loss_alone_pulls_a_perturbed_pose_back():
    """As test_bundle_adjustment_recovers_a_perturbed_pose, with an L1 loss on the DEPTH map alone (against the depth rendered
    at the true pose), Gaussians fixed: the pose leaves receive their gradient only through dL/dz and the depth term of
    dL/dalpha.  Without the feature the depth map carries no gradient at all."""
    from bags_raster import GaussianRasterizationSettings, GaussianRasterizer
    from bags_raster.synth import look_at_origin_camera, synth_scene
    dev = torch.device("cuda")
    W, H = 160, 120
    scene = {k: v.to(dev) for k, v in synth_scene(4000, 3, 2.0, 2).items()}
    P = scene["means3D"].shape[0]

    def render_depth(cam):
        st = GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
            bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam.get_world_view_transform(),
            projmatrix=cam.get_full_proj_transform(), intrinsic=cam.get_intrinsic(), sh_degree=2,
            campos=cam.get_camera_center(), prefiltered=False, debug=False, debug_iter=0, depth_weights_grad=True)
        img, radii, depth, weights, mean2D = GaussianRasterizer(st)(
            means3D=scene["means3D"], means2D=torch.zeros(P, 3, device=dev), means2D_densify=torch.zeros(P, 3, device=dev),
            shift_factors=torch.zeros(3, device=dev), shs=scene["shs"], colors_precomp=None, opacities=scene["opacities"],
            scales=scene["scales"], rotations=scene["rotations"], cov3D_precomp=None)
        return depth

    true_cam = look_at_origin_camera(W, H, device=dev)
    with torch.no_grad():
        target = render_depth(true_cam)
    cam = look_at_origin_camera(W, H, device=dev)
    with torch.no_grad():
        cam.delta_translation += torch.tensor([[0.06], [-0.04], [0.08]], device=dev)
        cam.delta_quaternion += torch.tensor([0.0, 0.01, -0.012, 0.008], device=dev)
    opt = torch.optim.Adam([{"params": [cam.delta_quaternion], "lr": 2e-3}, {"params": [cam.delta_translation], "lr": 5e-3}])

    def pose_err():
        return (cam.delta_translation.norm() + cam.delta_quaternion[1:].norm()).item()
    e0 = pose_err()
    losses = []
    for it in range(150):
        opt.zero_grad(set_to_none=True)
        loss = (render_depth(cam) - target).abs().mean()
        loss.backward()
        assert cam.delta_translation.grad is not None and torch.isfinite(cam.delta_translation.grad).all()
        assert float(cam.delta_translation.grad.abs().sum()) > 0
        opt.step()
        losses.append(loss.item())
    print(e0, pose_err(), losses[0], losses[-1])
    assert losses[-1] < 0.35 * losses[0], (losses[0], losses[-1])
    assert pose_err() < 0.5 * e0, (e0, pose_err())
