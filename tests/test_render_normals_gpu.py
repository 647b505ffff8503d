"""GPU checks of bags_raster.render_normals: the normal map against the operator called by hand and against the oracle's forward
with negative colours, the weights map against render()'s, one backward through normal_map_loss down to the Gaussians and the pose,
and the list path against the single-camera path."""
import pytest
import torch

from bags_raster import (GaussianRasterizer, PipelineParams, PoseBank, gaussian_normals, normal_map_loss, render, render_normals)
from bags_raster.gaussians import GaussianBag
from bags_raster.synth import look_at_origin_camera
from parity import assert_image_bars, compare
from scenes import hip_settings, make_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
W, H, P = 64, 48, 400


class _OneChain:
    """A camera whose chain is evaluated once, so that every route reads the SAME matrices."""

    def __init__(self, cam):
        self._cam, self._m = cam, None

    def __getattr__(self, n):
        return getattr(self._cam, n)

    def get_matrices(self, a=None, b=None):
        if self._m is None:
            self._m = self._cam.get_matrices(a, b)
        return self._m


def _scene():
    scene, _ = make_case(P, W, H, 2.0, 1, seed=3)
    return scene


def _bag(scene):
    return GaussianBag.from_activated({k: v.cpu() for k, v in scene.items()}, 1, device=DEV)


def test_the_normal_map_is_the_operator_with_the_normals_as_colours():
    scene = _scene()
    bag, cam = _bag(scene), _OneChain(look_at_origin_camera(W, H, device=DEV))
    pipe = PipelineParams()
    with torch.no_grad():
        out = render_normals(cam, bag, pipe, None)
        assert set(out) == {"normal", "weights", "depth", "radii"}
        assert out["normal"].shape == (3, H, W) and out["weights"].shape == (1, H, W) and out["radii"].shape == (P,)
        # by hand
        xyz, _, opacity, scaling, rotation = bag.activated(features=False)
        view, proj, intr, campos = cam.get_matrices(None, None)
        normals = gaussian_normals(rotation, bag._scaling, xyz, view)
        assert (normals < 0).any() and ((normals.norm(dim=1) - 1).abs() < 1e-5).all()
        st = hip_settings(cam, 1, DEV, tensors=dict(viewmatrix=view, projmatrix=proj, intrinsic=intr, campos=campos))
        img, radii, depth, weights, _ = GaussianRasterizer(st)(means3D=xyz, means2D=None, opacities=opacity, shift_factors=torch.zeros(3, device=DEV),
                                                               colors_precomp=normals, scales=scaling, rotations=rotation)
        assert torch.equal(out["normal"], img) and torch.equal(out["radii"], radii) and torch.equal(out["depth"], depth)
        assert torch.equal(out["weights"], weights) and (out["normal"] < 0).any() and (radii > 0).sum() > 100
        # the weights of a render() call on the same inputs
        res = render(cam, bag, pipe, torch.zeros(3, device=DEV), 0.0, None)
        assert torch.equal(out["weights"], res["weights"]) and torch.equal(out["depth"], res["depth"]) and torch.equal(out["radii"], res["radii"])
        # the activated scales order as the stored ones do: the same normals
        assert torch.equal(gaussian_normals(rotation, scaling, xyz, view), normals)


def test_the_normal_map_is_the_oracles_sum_of_weighted_normals():
    """sum_i w_i n_i from the oracle's forward with the normals as (negative) precomputed colours, at the project's image bar."""
    scene = _scene()
    cam = look_at_origin_camera(W, H)
    view = cam.get_world_view_transform().detach().to(DEV)
    normals = gaussian_normals(scene["rotations"].to(DEV), scene["scales"].to(DEV), scene["means3D"].to(DEV), view).cpu()
    assert (normals < 0).any()
    rep = compare(scene, cam, 1, colors=normals)
    print("\nrender_normals against the oracle: image %.2e (fp32 oracle %.2e, fp64 %.2e)  depth %.2e  weights %.2e"
          % (rep["image_max_err"], rep["image_max_err_fp32"], rep["image_max_err_fp64"], rep["depth_max_err"], rep["weights_max_err"]))
    assert_image_bars(rep)
    # and render_normals gives that image
    with torch.no_grad():
        out = render_normals(look_at_origin_camera(W, H, device=DEV), _bag(scene), PipelineParams(), None)
    from parity import run_hip
    img = run_hip(scene, cam, 1, colors=normals)[0][0]
    assert (out["normal"].cpu() - img).abs().max().item() <= 1e-5      # (the bag's activations round-trip through log / logit)


def test_one_backward_through_normal_map_loss_reaches_the_gaussians_and_the_pose():
    scene = _scene()
    bag, cam = _bag(scene), look_at_origin_camera(W, H, device=DEV)
    out = render_normals(cam, bag, PipelineParams(), None, depth_weights_grad=True)
    target = torch.zeros(3, H, W, device=DEV)
    target[2] = -1.0
    target[0] = 0.2
    loss, count = normal_map_loss(out["normal"], out["weights"], target, min_weight=0.05, min_norm=0.02)
    assert count.item() > 50
    loss.sum().backward()
    torch.cuda.synchronize()
    leaves = {"rotations": bag._rotation, "xyz": bag._xyz, "opacity": bag._opacity, "delta_translation": cam.delta_translation,
              "delta_quaternion": cam.delta_quaternion}
    for n, t in leaves.items():
        assert t.grad is not None and torch.isfinite(t.grad).all() and t.grad.abs().max().item() > 0, n


def test_the_list_path_gives_the_bits_of_the_single_camera_path():
    scene = _scene()
    bag = _bag(scene)
    bank = PoseBank.from_cameras([look_at_origin_camera(W, H, T=torch.tensor([0.1 * i, 0.0, 4.0 + 0.3 * i])) for i in range(3)], device=DEV)
    cams = [look_at_origin_camera(W, H, device=DEV, T=torch.tensor([0.1 * i, -0.05 * i, 4.0 + 0.3 * i])) for i in range(3)]
    with torch.no_grad():
        many = render_normals(cams, bag, PipelineParams(), None)
        assert isinstance(many, list) and len(many) == 3
        for cam, m in zip(cams, many):
            one = render_normals(cam, bag, PipelineParams(), None)
            assert isinstance(one, dict)
            for n in ("normal", "weights", "depth", "radii"):
                assert torch.equal(one[n], m[n]), n
        assert not torch.equal(many[0]["normal"], many[1]["normal"])
        # the cameras of one PoseBank: one chain launch for the list
        rows = [bank.camera(i) for i in range(3)]
        banked = render_normals(rows, bag, PipelineParams(), None)
        for i, m in enumerate(banked):
            one = render_normals(rows[i], bag, PipelineParams(), None)
            for n in ("normal", "weights", "depth", "radii"):
                assert torch.equal(one[n], m[n]), n
