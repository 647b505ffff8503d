"""GPU checks of antialiased rendering: bags_raster.antialias_opacity (csrc/antialias.hip) against its PyTorch statement in float32
and float64 on the named cases of tests/antialias_cases.py, the independence and repeatability of its outputs, and
GaussianRasterizationSettings(antialiasing=True) against the same function composed by hand in front of the operator."""
import math

import pytest
import torch

import antialias_cases as A
import bags_raster
from bags_raster import GaussianRasterizer, PipelineParams, antialias_opacity, debug_views
from bags_raster.gaussians import GaussianBag
from scenes import hip_settings, make_case, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64
SLACK = 3.0                                       # parity.assert_ill_conditioned: the project's slack for ill-conditioned cases

# (case, cov3D_precomp instead of the scale pair, scale_modifier, clamp_grad)
VARIANTS = [(n, False, 1.0, "stock") for n in A.CASES] + \
           [(n, True, 1.0, "stock") for n in ("generic", "inside_shift", "flat")] + \
           [("generic", False, 1.7, "stock"), ("inside_shift", True, 1.7, "stock"), ("subpixel", False, 1.7, "exact"),
            ("inside", False, 1.0, "exact"), ("inside_shift", False, 1.7, "exact"), ("inside_shift", True, 1.0, "exact")]
IDS = ["%s-%s-%g-%s" % (n, "cov" if c else "pair", m, g) for n, c, m, g in VARIANTS]


def _hip(name, P=A.P_FULL, cov=False, mod=1.0, clamp="stock", row_mask=None):
    out, grads = A.forward_backward(antialias_opacity, name, F32, DEV, P, cov, mod, clamp, row_mask)
    torch.cuda.synchronize()
    return out.cpu(), {n: g.cpu() for n, g in grads.items()}


# ---------------------------------------------------------------------------------------------------------------- 6. forward, 7. backward
@pytest.mark.parametrize("name,cov,mod,clamp", VARIANTS, ids=IDS)
def test_forward_and_backward_against_the_statement(name, cov, mod, clamp):
    """Well-conditioned cases: every row of the output within 1e-5 (1 + |x|) of the float32 statement AND of float64, every
    gradient tensor within 1e-4 (scenes.rel_err) of float64 autograd.  `flat`: the kernel may be SLACK x as far from float64 as
    the float32 statement is.  `needles`: the same, with the rows whose floor decision differs between float32 and float64 taken
    out of all three sides (their cotangent is zero); the cases module bounds how many those are.

    Measured on an MI355X (the test prints every figure; table in profiles/antialias/NOTES.md): the forward equals the float32
    statement bit for bit on every row of every case; worst gradient tensor against float64, kernel (float32 statement):
    generic 1.5e-6 (8.7e-6), small 1.5e-7 (2.4e-7), subpixel 1.8e-7 (1.8e-7), inside 6.5e-7 (4.9e-5), inside_shift 5.8e-7 (1.2e-4),
    flat 1.63e-3 (1.63e-3), needles intrinsic 1.0e-1 (8.0e-2) with 5 rows left out."""
    masked = name == "needles"
    flips = A.floor_flips(name, A.P_FULL, cov, mod)
    if masked:
        assert int(flips.sum()) <= A.P_FULL // 100
    o64, g64 = A.reference(name, F64, A.P_FULL, cov, mod, clamp, masked)
    o32, g32 = A.reference(name, F32, A.P_FULL, cov, mod, clamp, masked)
    out, grads = _hip(name, A.P_FULL, cov, mod, clamp, ~flips if masked else None)
    assert out.shape == (A.P_FULL, 1) and out.dtype == F32 and torch.isfinite(out).all()
    keep = ~flips if masked else torch.ones_like(flips)
    d32 = (out.double() - o32.double()).abs()[keep]
    d64 = (out.double() - o64).abs()[keep]
    ref = (o32.double() - o64).abs()[keep].max().item()
    print("\n%s forward: max |hip - f32| %.3e  |hip - f64| %.3e  |f32 - f64| %.3e  bitwise equal to f32 on %d of %d rows"
          % (name, d32.max().item(), d64.max().item(), ref, int((out == o32)[keep].sum()), int(keep.sum())))
    if name in A.WELL:
        assert (d32 <= 1e-5 * (1 + o32.double().abs()[keep])).all() and (d64 <= 1e-5 * (1 + o64.abs()[keep])).all()
    else:
        assert d64.max().item() <= SLACK * ref + 1e-5
    assert set(grads) == set(g64)
    errs = {n: (rel_err(grads[n], g64[n]), rel_err(g32[n], g64[n])) for n in g64}
    print("%s backward: " % name + "  ".join("%s %.2e (f32 %.2e)" % (n, a, b) for n, (a, b) in errs.items()))
    for n, (err, ref32) in errs.items():
        assert torch.isfinite(grads[n]).all(), n
        if name in A.WELL:
            assert err <= 1e-4, (n, err)
        else:
            assert err <= SLACK * ref32 + 1e-4, (n, err, ref32)
    # what nothing depends on is written as zeros, not left as it was
    assert grads["viewmatrix"][:, 3].abs().max().item() == 0.0
    k = grads["intrinsic"].reshape(16)
    assert k[[i for i in range(16) if i not in (0, 5)]].abs().max().item() == 0.0 and k[0] != 0 and k[5] != 0


@pytest.mark.parametrize("P", A.SIZES)
@pytest.mark.parametrize("name", ("generic", "inside_shift"))
def test_cloud_sizes_either_side_of_a_workgroup(name, P):
    o64, g64 = A.reference(name, F64, P)
    out, grads = _hip(name, P)
    assert out.shape == (P, 1) and ((out.double() - o64).abs() <= 1e-5 * (1 + o64.abs())).all()
    for n in g64:
        assert tuple(grads[n].shape) == tuple(g64[n].shape)
        if g64[n].abs().max().item() > 0:                    # (P = 1: a single row may sit where a gradient is zero)
            assert rel_err(grads[n], g64[n]) <= 1e-4, (n, rel_err(grads[n], g64[n]))
        else:
            assert grads[n].abs().max().item() == 0.0, n


def test_dead_rows_give_the_opacity_gradient_and_nothing_else():
    """`subpixel` has 542 rows on the floor and `inside` 196 behind the near plane: their rows of every per-Gaussian gradient are
    exactly zero, dL/dopacity is g h, and the pose sums are finite."""
    for name in ("subpixel", "inside"):
        d = A._decisions(name, F32, A.P_FULL, False, 1.0)
        dead = d["culled"] | d["floor"]
        out, grads = _hip(name)
        assert int(dead.sum()) > 190
        for n in ("means3D", "scales", "rotations"):
            assert grads[n][dead].abs().max().item() == 0.0 and grads[n][~dead].abs().max().item() > 0.0, (name, n)
        h = torch.where(d["culled"], torch.ones(()), torch.where(d["floor"], torch.tensor(math.sqrt(A.FLOOR)), d["h"])).reshape(-1, 1)
        assert (grads["opacities"] - A.cotangent(A.P_FULL).float() * h).abs().max().item() <= 1e-6
        assert torch.equal(out[d["culled"]], A.case(name)["opacities"][d["culled"]])
        assert all(torch.isfinite(grads[n]).all() for n in ("viewmatrix", "intrinsic"))


# ---------------------------------------------------------------------------------------------------------------- 8. subsets
def _with_grads(name, wanted, cov=False):
    lv = A.leaves(name, F32, DEV, cov=cov)
    for n, t in lv.items():
        t.requires_grad_(n in wanted)
    out = A.run(antialias_opacity, name, lv)
    gs = torch.autograd.grad(out, [lv[n] for n in wanted], A.cotangent(A.P_FULL).to(DEV, F32))
    return dict(zip(wanted, gs))


@pytest.mark.parametrize("cov", (False, True), ids=("pair", "cov"))
def test_a_wanted_output_does_not_depend_on_which_others_are_wanted(cov):
    name = "inside_shift"
    source = ("cov3D_precomp",) if cov else ("scales", "rotations")
    everything = ("means3D", "opacities", "viewmatrix", "intrinsic", "shift_factors") + source
    full = _with_grads(name, everything, cov)
    subsets = [("viewmatrix", "intrinsic", "shift_factors"), ("opacities",), ("intrinsic",), ("means3D",),
               tuple(n for n in everything if n != "rotations")]
    for wanted in subsets:
        part = _with_grads(name, wanted, cov)
        for n in wanted:
            assert torch.equal(part[n], full[n]), (wanted, n)


# ---------------------------------------------------------------------------------------------------------------- 9. reproducible
def test_two_runs_give_the_same_bits():
    a_out, a = _hip("inside_shift")
    b_out, b = _hip("inside_shift")
    assert torch.equal(a_out, b_out)
    for n in a:
        assert torch.equal(a[n], b[n]), n
    assert a["viewmatrix"].abs().max().item() > 0 and a["shift_factors"].abs().max().item() > 0


def test_one_row_and_no_rows():
    out, grads = _hip("generic", 1)
    assert out.shape == (1, 1) and 0 < out.item() < A.case("generic")["opacities"][0].item()
    lv = A.leaves("inside_shift", F32, DEV, P=0)
    out = A.run(antialias_opacity, "inside_shift", lv)
    assert out.shape == (0, 1)
    out.sum().backward()
    torch.cuda.synchronize()
    for n, t in lv.items():
        assert t.grad is not None and t.grad.shape == t.shape and (t.grad.numel() == 0 or t.grad.abs().max().item() == 0.0), n
    with torch.no_grad():
        assert A.run(antialias_opacity, "inside_shift", lv).shape == (0, 1)


# ---------------------------------------------------------------------------------------------------------------- 10. composition
def _scene(seed=0):
    scene, cam = make_case(600, 64, 48, 0.25, 1, seed=seed)
    settings = hip_settings(cam, 1, DEV)
    return {k: v.to(DEV) for k, v in scene.items()}, cam, settings


def _operator_route(settings, scene, shift, by_hand, g_img, cov=False):
    """Image, radii, depth, weights and every gradient of one forward + backward; by_hand: antialias_opacity composed in front of
    a plain rasterizer instead of the settings' switch."""
    lv = {k: v.detach().clone().requires_grad_(True) for k, v in scene.items()}
    cam_lv = {k: getattr(settings, k).detach().clone().requires_grad_(True) for k in ("viewmatrix", "projmatrix", "intrinsic", "campos")}
    sf = shift.detach().clone().requires_grad_(True)
    st = settings._replace(antialiasing=not by_hand, **cam_lv)
    src = dict(cov3D_precomp=bags_raster.gaussians.covariance_from_scaling_rotation(lv["scales"], st.scale_modifier, lv["rotations"])) if cov \
        else dict(scales=lv["scales"], rotations=lv["rotations"])
    opac = lv["opacities"]
    if by_hand:
        opac = antialias_opacity(lv["means3D"], opac, st.viewmatrix, st.intrinsic, (st.image_height, st.image_width), (st.tanfovx, st.tanfovy),
                                 shift_factors=sf, scale_modifier=st.scale_modifier, clamp_grad=st.clamp_grad, **src)
    m2d = torch.zeros_like(lv["means3D"], requires_grad=True)
    img, radii, depth, weights, mean2D = GaussianRasterizer(st)(means3D=lv["means3D"], means2D=m2d, opacities=opac, shift_factors=sf,
                                                                shs=lv["shs"], **src)
    (img * g_img).sum().backward()
    torch.cuda.synchronize()
    grads = {k: v.grad for k, v in {**lv, **cam_lv, "shift_factors": sf, "means2D": m2d}.items()}
    return dict(img=img.detach(), radii=radii, depth=depth.detach(), weights=weights.detach(), mean2D=mean2D.detach()), grads


@pytest.mark.parametrize("cov", (False, True), ids=("pair", "cov"))
def test_the_setting_is_the_function_in_front_of_the_operator(cov):
    scene, cam, settings = _scene()
    g_img = torch.randn(3, 48, 64, generator=torch.Generator().manual_seed(7)).to(DEV)
    shift = torch.tensor([0.02, -0.01, 0.005], device=DEV)
    a_out, a = _operator_route(settings, scene, shift, False, g_img, cov)
    b_out, b = _operator_route(settings, scene, shift, True, g_img, cov)
    for n in a_out:
        assert torch.equal(a_out[n], b_out[n]), n
    for n in a:
        assert a[n] is not None and torch.equal(a[n], b[n]), n
    assert (a_out["radii"] > 0).sum() > 100 and a["opacities"].abs().max().item() > 0
    # debug_views applies the factor too (under no_grad)
    with torch.no_grad():
        o_aa = antialias_opacity(scene["means3D"], scene["opacities"], settings.viewmatrix, settings.intrinsic, (48, 64),
                                 (settings.tanfovx, settings.tanfovy), scales=scene["scales"], rotations=scene["rotations"], shift_factors=shift)
    dv = lambda st, o: debug_views(st, scene["means3D"], None, shift, scene["shs"], None, o, scene["scales"], scene["rotations"], None)       # noqa: E731
    v_aa, v_hand, v_plain = dv(settings._replace(antialiasing=True), scene["opacities"]), dv(settings, o_aa), dv(settings, scene["opacities"])
    assert v_aa["num_rendered"] == v_hand["num_rendered"] <= v_plain["num_rendered"]
    assert torch.equal(v_aa["outputs"][0], v_hand["outputs"][0]) and not torch.equal(v_aa["outputs"][0], v_plain["outputs"][0])


class _OneChain:
    """A camera whose chain is evaluated once, so that the function and the operator of the by-hand route read the SAME matrices."""

    def __init__(self, cam):
        self._cam, self._m = cam, None

    def __getattr__(self, n):
        return getattr(self._cam, n)

    def get_matrices(self, a=None, b=None):
        if self._m is None:
            self._m = self._cam.get_matrices(a, b)
        return self._m


class _ByHand:
    """A Gaussian set whose activated opacity has been through antialias_opacity."""

    def __init__(self, bag, cam, mod):
        self._bag, self._cam, self._mod = bag, cam, mod

    def __getattr__(self, n):
        return getattr(self._bag, n)

    def activated(self, features=True):
        xyz, feats, opac, scaling, rotation = self._bag.activated(features=features)
        view, _, intr, _ = self._cam.get_matrices(None, None)
        c = self._cam
        opac = antialias_opacity(xyz, opac, view, intr, (int(c.image_height), int(c.image_width)), (math.tan(c.FoVx * 0.5), math.tan(c.FoVy * 0.5)),
                                 scales=scaling, rotations=rotation, scale_modifier=self._mod)
        return xyz, feats, opac, scaling, rotation


def test_render_passes_the_pipeline_switch_on():
    from bags_raster.render import render
    from bags_raster.synth import look_at_origin_camera
    from types import SimpleNamespace
    scene, _, _ = _scene()
    g_img = torch.randn(3, 48, 64, generator=torch.Generator().manual_seed(8)).to(DEV)
    bg = torch.zeros(3, device=DEV)

    def route(pipe, by_hand):
        bag = GaussianBag.from_activated({k: v.cpu() for k, v in scene.items()}, 1, device=DEV)
        cam = _OneChain(look_at_origin_camera(64, 48, device=DEV))
        res = render(cam, _ByHand(bag, cam, 0.9) if by_hand else bag, pipe, bg, 0.0, None, hybrid=False, scaling_modifier=0.9)
        (res["render"] * g_img).sum().backward()
        torch.cuda.synchronize()
        cam_leaves = [cam.delta_translation, cam.delta_quaternion, cam.learnable_fovx, cam.learnable_fovy]
        return res, [t.grad for t in bag.leaves() + cam_leaves]
    aa, g_aa = route(PipelineParams(antialiasing=True), False)
    hand, g_hand = route(PipelineParams(), True)
    plain, _ = route(SimpleNamespace(convert_SHs_python=False, compute_cov3D_python=False, debug=False), False)     # a reference `pipe`: no attribute
    for n in ("render", "radii", "depth", "weights"):
        assert torch.equal(aa[n], hand[n]), n
    for i, (x, y) in enumerate(zip(g_aa, g_hand)):
        assert (x is None) == (y is None) and (x is None or torch.equal(x, y)), i
    assert sum(g is not None for g in g_aa) >= 7
    assert not torch.equal(aa["render"], plain["render"]) and (aa["weights"] <= plain["weights"] + 1e-6).all()


# ---------------------------------------------------------------------------------------------------------------- 11. direction
def test_antialiasing_only_takes_energy_away():
    """`subpixel` at 64x48: every alpha shrinks (h <= 1), so 1 - prod(1 - alpha) shrinks on every pixel, and under
    tile_bounds="opacity" the alpha >= 1/255 reach of a splat shrinks with its opacity: no instance list gets longer."""
    c = A.case("subpixel")
    scene, cam = make_case(A.P_FULL, 64, 48, 1.0, 0, seed=2)
    st = hip_settings(cam, 0, DEV, tile_bounds="opacity")
    t = {n: c[n].to(DEV) for n in ("means3D", "opacities", "scales", "rotations")}
    shs = scene["shs"].to(DEV)
    assert torch.equal(t["means3D"].cpu(), scene["means3D"])
    dv = lambda s: debug_views(s, t["means3D"], None, None, shs, None, t["opacities"], t["scales"], t["rotations"], None)       # noqa: E731
    plain, aa = dv(st), dv(st._replace(antialiasing=True))
    w_plain, w_aa = plain["outputs"][3], aa["outputs"][3]
    assert w_plain.max().item() > 1e-3                                    # something is rendered
    assert (w_aa <= w_plain + 1e-6).all() and w_aa.sum().item() < 0.5 * w_plain.sum().item()
    assert aa["num_rendered"] <= plain["num_rendered"]
    assert (aa["tiles_touched"] <= plain["tiles_touched"]).all()


# ---------------------------------------------------------------------------------------------------------------- 12. errors
def test_refusals_name_the_operator():
    lv = {n: t.detach() for n, t in A.leaves("generic", F32, DEV, P=5).items()}
    c = A.case("generic")
    base = dict(scales=lv["scales"], rotations=lv["rotations"], cov3D_precomp=None)

    def call(means=lv["means3D"], opac=lv["opacities"], view=lv["viewmatrix"], intr=lv["intrinsic"], hw=c["image_hw"], **kw):
        a = dict(base)
        a.update(kw)
        return antialias_opacity(means, opac, view, intr, hw, c["tanfov"], **a)
    assert call().shape == (5, 1)
    with pytest.raises(NotImplementedError, match="antialias_opacity runs only on an AMD GPU.*antialias_opacity_torch"):
        call(means=lv["means3D"].cpu())
    with pytest.raises(NotImplementedError, match="antialias_opacity runs only on an AMD GPU"):
        call(shift_factors=torch.zeros(3))
    for kw in (dict(means=lv["means3D"][:, :2]), dict(opac=lv["opacities"][:4]), dict(view=lv["viewmatrix"][:3]), dict(intr=lv["intrinsic"].reshape(16)),
               dict(scales=lv["scales"][:4]), dict(rotations=lv["rotations"][:, :3]), dict(shift_factors=torch.zeros(4, device=DEV)),
               dict(scales=None, rotations=None, cov3D_precomp=torch.zeros(5, 5, device=DEV)), dict(hw=(0, 64))):
        with pytest.raises(ValueError, match="antialias_opacity: "):
            call(**kw)
    for kw in (dict(scales=None, rotations=None), dict(rotations=None), dict(cov3D_precomp=torch.zeros(5, 6, device=DEV))):
        with pytest.raises(ValueError, match="antialias_opacity: provide exactly one of either scale/rotation pair"):
            call(**kw)
    with pytest.raises(TypeError, match="antialias_opacity: means3D must be float32"):
        call(means=lv["means3D"].double())
    with pytest.raises(ValueError, match="antialias_opacity: clamp_grad"):
        call(clamp_grad="both")
