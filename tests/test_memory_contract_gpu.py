"""Every entry point of include/bags_raster.h held to its memory contract: outputs, gradients and workspaces come out of the middle
of dirty buffers whose borders are read back (tests/fenced.py; tests/test_fenced_cpu.py holds that helper to its word).

One table, ROWS: a name, ``run(f)`` -- inputs from the existing ``*_cases`` / ``*_reference`` modules and the run helpers of the
operation's own test file, forward AND backward through the public wrapper, every output and gradient returned -- and what the row's
workspaces promise.  One parametrised test per property:

  1. nothing outside a buffer is written               under dirt 0xA5 and under 0xFF every band is intact
  2. nothing depends on what the memory held           plain run, 0xA5 run and 0xFF run are torch.equal, tensor by tensor
  3. the interception is real                          nothing passed through unfenced, the package's own allocations were fenced,
                                                       the op's workspace was served
  4. a rounded-base workspace may start anywhere       shift 1: same bits, bands intact
  5. an as-given workspace is taken at its alignment   shift 16 (the loss: also 4): same bits; off it: RuntimeError, bands intact
  6. one byte short is refused                         shrink 1: RuntimeError naming the buffer, bands intact

The values themselves are held to float64 by each operation's own test file; here a wrong value can only show as a difference
between the three runs.  For 5 and 6 the host checks of csrc/api.hip were read: each refuses before its first launch, so no kernel
runs on a base or a size the header forbids (the loss entry points got their alignment check with this file).

profiles/memory_contract/NOTES.md lists the rows against the size functions of the header, with the counts this file prints."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from bags_raster import _lib as L
from fenced import fenced

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
DIRTS = (0xA5, 0xFF)

ROUNDED, GIVEN16, GIVEN4 = "rounded", "as given, 16 bytes", "as given, 4 bytes"


class _Plain:
    """What ``run(f)`` is handed outside a fence: the same interface, ordinary memory."""
    @staticmethod
    def copy(t):
        return t.detach().clone().requires_grad_(t.requires_grad)


PLAIN = _Plain()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _fence_optimizer(f, opt, bag=None):
    """The parameters, gradients and moments of ``opt`` (and the statistics of ``bag``) re-homed by ``f.copy``: what the in-place
    entry points write.  The parameter objects stay the same."""
    for group in opt.param_groups:
        for p in group["params"]:
            p.data = f.copy(p.data)
            if p.grad is not None:
                p.grad = f.copy(p.grad)
            st = opt.state.get(p)
            if st:
                for k in ("exp_avg", "exp_avg_sq"):
                    if k in st:
                        st[k] = f.copy(st[k])
    if bag is not None:
        for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
            setattr(bag, k, f.copy(getattr(bag, k)))


def _opt_tensors(opt):
    out = []
    for group in opt.param_groups:
        p = group["params"][0]
        st = opt.state.get(p) or {}
        out += [p.detach(), st.get("exp_avg"), st.get("exp_avg_sq")]
    return out


# ------------------------------------------------------------------------------------------------------------------ the rasterizer
def _cot(H, W, seed=5, C_=3):
    return torch.randn(C_, H, W, generator=_gen(seed))


def _raster(P, W, H, sm, deg, **kw):
    """The exact two-phase forward (no capacity hint yet), then the speculative one (hint present, the backward's buffers
    preallocated), each with backward and bags_debug_views.  Workspace calls: geom 0, image 1, binning 2, backward 3, debug_views
    4-6; then 7, 8, 9, 10 and 11-13."""
    def run(f):
        from bags_raster import rasterizer as R
        from parity import run_hip
        from scenes import make_case
        scene, cam = make_case(P, W, H, sm, deg)
        R._capacity_hint.clear()
        a = run_hip(scene, cam, deg, _cot(H, W), **kw)
        b = run_hip(scene, cam, deg, _cot(H, W), **kw)
        return [a, b]
    return run


# (Call 10, the backward workspace the speculative forward preallocates, is sized for the CAPACITY, above the true count the backward
# checks it against: one byte short of that still holds every record, and is rightly accepted.)
RASTER_SHORT = ((0, "geom buffer"), (1, "image buffer"), (2, "binning buffer"), (3, "backward workspace"), (9, "binning buffer"))


def _raster_extras(f):
    """depth_weights_grad: the depth and weights maps with cotangents of their own (bags_backward_ex)."""
    from bags_raster import rasterizer as R
    from depth_oracle import run_hip_ex
    from scenes import make_case
    scene, cam = make_case(1000, 128, 96, 2.0, 3)
    R._capacity_hint.clear()
    return list(run_hip_ex(scene, cam, 3, _cot(96, 128, 6), _cot(96, 128, 7, 1), _cot(96, 128, 8, 1)))


def _raster_empty(f):
    """P = 0: no prepare phase runs; the background comes out, the camera tensors get zeros."""
    from bags_raster import GaussianRasterizer
    from bags_raster.synth import look_at_origin_camera
    from scenes import camera_tensors, hip_settings
    dev = torch.device(DEV)
    out = []
    for binning in ("auto", "radix"):
        cam = look_at_origin_camera(80, 48)
        ct = {k: v.clone().requires_grad_(True) for k, v in camera_tensors(cam, dev).items()}
        st = hip_settings(cam, 2, dev, bg=torch.tensor([0.1, 0.5, 0.9]), tensors=ct, binning=binning)
        z = lambda *s: torch.zeros(*s, device=dev)                      # noqa: E731
        o = GaussianRasterizer(st)(means3D=z(0, 3), means2D=z(0, 3), means2D_densify=z(0, 3), shift_factors=z(3), shs=z(0, 9, 3),
                                   colors_precomp=None, opacities=z(0, 1), scales=z(0, 3), rotations=z(0, 4), cov3D_precomp=None)
        (o[0] * _cot(48, 80).to(dev)).sum().backward()
        out += [o[0].detach(), o[2].detach(), o[3].detach()] + [v.grad for v in ct.values()]
    return out


def _speculative(lazy):
    """The case of test_speculative_forward_matches_exact_and_recovers_from_overflow: a call that sets the capacity hint, then six
    times the scales -- several times more instances than the binning buffer that was sized from the guess.  Default mode redoes the
    second phase on an exact buffer; HOST_WAIT = "lazy" raises SpeculationOverflow at the backward's entry and the retry fits."""
    def run(f):
        from bags_raster import rasterizer as R
        from parity import run_hip
        from scenes import make_case
        scene, cam = make_case(3000, 160, 128, 1.0, 2, seed=31)
        big = dict(scene)
        big["scales"] = scene["scales"] * 6.0
        g = _cot(128, 160)
        saved = (R.HOST_WAIT, R.LAZY_RECOVER)
        try:
            R.HOST_WAIT, R.LAZY_RECOVER = ("lazy" if lazy else "forward"), False
            R._capacity_hint.clear()
            first = run_hip(scene, cam, 2, g)
            assert R._capacity_hint, "hint not recorded"
            if lazy:
                with pytest.raises(R.SpeculationOverflow):
                    run_hip(big, cam, 2, g)
            over = run_hip(big, cam, 2, g)
            assert over[2]["num_rendered"] > 6 * first[2]["num_rendered"]
        finally:
            R.HOST_WAIT, R.LAZY_RECOVER = saved
            R._capacity_hint.clear()
        return [first, over]
    return run


def _render_step(f):
    """render_views and render_normals of the five PoseBank cameras of tests/step_cases.py (40 x 72: no multiple of the 16 x 16 tile),
    through the fused activations, the SH colours of all views, gaussian_normals and the operator, and back."""
    import test_step_gpu as TS
    o = TS._objects()
    maps, views, intrinsics = TS._forward(o)
    flat = [t for k in sorted(maps) for t in maps[k]]
    cots = [torch.randn(t.shape, generator=_gen(40 + i)).to(DEV) for i, t in enumerate(flat)]
    torch.autograd.backward(flat + [views], cots + [torch.randn(views.shape, generator=_gen(39)).to(DEV)])
    return [t.detach() for t in flat] + [views.detach(), intrinsics.detach()] + [t.grad for t in o.bag.leaves()] + [o.bank.leaves.grad]


def _factored_sh(f):
    """rasterizer.FactoredSH: every view's backward writes its (P,3) dL/dcolour, finish() forms the SH rows of the step in one
    launch (bags_sh_gradient_from_views); a second step accumulates on top.  P = 257, features_dc / features_rest, M = 16."""
    from bags_raster import GaussianRasterizationSettings, GaussianRasterizer, rasterizer as R
    from bags_raster.synth import sphere_views, synth_scene
    from scenes import camera_tensors
    dev = torch.device(DEV)
    P, W, H, V = 257, 72, 40, 2
    scene = synth_scene(P, 11, 1.5, 3)
    cams = sphere_views(V, W, H, noise=0.05)
    saved = (R.ACCUMULATE_IN_PLACE, R.FACTORED_SH)
    R.ACCUMULATE_IN_PLACE = True
    try:
        leaves = {k: v.to(dev).clone().requires_grad_(True) for k, v in scene.items() if k != "shs"}
        dc = scene["shs"][:, :1].contiguous().to(dev).requires_grad_(True)
        rest = scene["shs"][:, 1:].contiguous().to(dev).requires_grad_(True)
        for step in range(2):
            fs = R.FACTORED_SH = R.FactoredSH()
            for v, cam in enumerate(cams):
                ct = {k: t.clone().requires_grad_(True) for k, t in camera_tensors(cam, dev).items()}
                st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
                                                   bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=ct["viewmatrix"],
                                                   projmatrix=ct["projmatrix"], intrinsic=ct["intrinsic"], sh_degree=3, campos=ct["campos"])
                img = GaussianRasterizer(st)(means3D=leaves["means3D"], means2D=torch.zeros(P, 3, device=dev, requires_grad=True), shs=dc,
                                             shs_rest=rest, opacities=leaves["opacities"], scales=leaves["scales"], rotations=leaves["rotations"])[0]
                img.backward(_cot(H, W, 30 + v).to(dev))
            R.FACTORED_SH = None
            fs.finish(leaves["means3D"], dc, rest)
        return [t.grad for t in leaves.values()] + [dc.grad, rest.grad]
    finally:
        R.ACCUMULATE_IN_PLACE, R.FACTORED_SH = saved


# ------------------------------------------------------------------------------------------------------------------ losses on images
def _loss(shape):
    """fused_l1_ssim and fused_photometric_loss; (3,33,31) takes the scalar path, (3,40,44) the vector path (W % 4 == 0)."""
    def run(f):
        import loss_cases as LC
        from bags_raster.loss import fused_l1_ssim, fused_photometric_loss
        a, b = LC.make_pair("noise", shape)
        at, bt = torch.from_numpy(a).to(DEV).requires_grad_(True), torch.from_numpy(b).to(DEV)
        l1, s = fused_l1_ssim(at, bt)
        torch.autograd.backward([l1, s], [torch.tensor(0.8, device=DEV), torch.tensor(-0.2, device=DEV)])
        g1, at.grad = at.grad, None
        loss, t1, t2 = fused_photometric_loss(at, bt, 0.2, return_terms=True)
        loss.backward()
        return [l1.detach(), s.detach(), g1, loss.detach(), t1, t2, at.grad]
    return run


def _depth_prior(mode, space):
    def run(f):
        import depth_prior_cases as P_
        import test_depth_prior_gpu as T
        return list(T._run(P_.make_case(17, 67, 17, mode, space)))
    return run


def _normal_prior(f):
    import normal_prior_cases as P_
    import test_normal_prior_gpu as T
    from bags_raster import depth_to_normal
    c = P_.make_case(17, 67, 17, "cos")
    n, ok = depth_to_normal(T._place(c["D"][0], False), T._place(c["A"][0], False), c["pinhole"][0], min_weight=P_.MIN_WEIGHT, max_jump=P_.MAX_JUMP)
    return list(T._run(c)) + list(T._run(P_.make_case(25, 66, 2, "l1"))) + [n, ok]


def _correspondence(f):
    import correspondence_cases as P_
    import test_correspondence_gpu as T
    from bags_raster import reproject_pixels
    c = P_.make_case(17, 67, 17, 1.0)
    proj, ok = reproject_pixels(T._place(c["D"][0], False), T._place(c["A"][0], False), c["Vi"][0].to(DEV), c["Vj"][0].to(DEV), c["pin_i"][0],
                                c["pin_j"][0], (17, 67), min_weight=P_.MIN_WEIGHT, min_depth=P_.MIN_DEPTH)
    return list(T._run(c)) + [proj, ok]


def _warp(f):
    import test_warp_gpu as T
    import warp_cases as P_
    from bags_raster import warp_image
    c = P_.make_case(17, 67, 17, 3, 1e-3)
    k = 0
    maps = (T._place(c["D_dst"][k], False), T._place(c["A_dst"][k], False)) if bool(c["has_dst"][k]) else (None, None)
    out, ok = warp_image(T._place(c["D"][k], False), T._place(c["A"][k], False), c["Vi"][k].to(DEV), c["Vj"][k].to(DEV), T._place(c["image"][k], False),
                         c["pin_i"][k], c["pin_j"][k], *maps, occlusion=P_.OCCLUSION, min_weight=P_.MIN_WEIGHT, min_depth=P_.MIN_DEPTH)
    return list(T._run(c)) + [out, ok]


def _normal_map(f):
    import test_normal_map_gpu as T
    out = []
    for name, H, W, V, mode, masked in (("generic", 33, 70, 17, "cos", True), ("holes", 33, 70, 5, "l1", True), ("generic", 5, 7, 1, "l1", False)):
        out.append(T._hip(name, H, W, V, mode, masked))
    return out


def _smooth(normals):
    def run(f):
        import smooth_cases as M
        import test_smooth_gpu as T
        cfgs = (M.normal_configs if normals else M.depth_configs)(0.0)
        return [T._hip("generic", 33, 70, 17, cfgs[0], normals), T._hip("generic", 33, 70, 17, cfgs[1], normals),
                T._hip("generic", 5, 7, 1, cfgs[3], normals)]
    return run


def _appearance(f):
    import appearance_cases as A
    import test_appearance_gpu as T
    c = A.make_case(17, 67, 17)
    return list(T._run(c)) + list(T._run(c, stacked=True, views=[0, 3, 1]))


def _bilagrid(f):
    import bilagrid_cases as B
    import test_bilagrid_gpu as T
    from bags_raster import bilagrid_tv_loss
    c = B.make_case((5, 4, 3), 21, 67, 17)
    grids = c["grids"].to(DEV).requires_grad_(True)
    tv = bilagrid_tv_loss(grids)
    tv.backward()
    return list(T._run(c)) + list(T._run(c, path=T.DIRECT, views=[2, 0])) + [tv.detach(), grids.grad]


# ------------------------------------------------------------------------------------------------------------------ per Gaussian
def _gaussian_reg(P):
    def run(f):
        import gaussian_reg_cases as G
        import test_gaussian_reg_gpu as T
        return [T._run(G.make_case(P, filtered, selected)) for filtered, selected in ((True, True), (False, False))]
    return run


def _gaussian_normals(P, V):
    def run(f):
        import test_gaussian_normals_gpu as T
        return list(T._hip("generic", P, V))
    return run


def _antialias(P):
    def run(f):
        import test_antialias_gpu as T
        return list(T._hip("generic", P)) + list(T._hip("inside_shift", P, cov=True, mod=1.7, clamp="exact"))
    return run


def _filter3d(P):
    def run(f):
        import filter3d_cases as F
        import test_filter3d_gpu as T
        return [T._hip(F.points("ring", 17)[:P], 17), T._hip(F.points("behind", 70)[:P], 70)]
    return run


def _activations(P, deg):
    def run(f):
        from bags_raster.gaussians import GaussianBag
        from bags_raster.synth import synth_scene
        pc = GaussianBag.from_activated(synth_scene(P, 9, 0.5, deg), deg, device=DEV)
        got = list(pc.activated())
        g = _gen(2)
        torch.autograd.backward(got[1:], [torch.randn(t.shape, generator=g).to(DEV) for t in got[1:]])
        return [t.detach() for t in got] + [t.grad for t in pc.leaves()]
    return run


def _activations_filtered(P):
    def run(f):
        import filter3d_cases as F
        import test_filter3d_gpu as T
        from bags_raster.gaussians import fused_activations
        lv = T._leaves(P, F32, DEV)
        outs = fused_activations(lv["features_dc"], lv["features_rest"], lv["opacity"], lv["scaling"], lv["rotation"], F.filter_values("ring", P).to(DEV))
        T._backward(outs[1], outs[2], P, "both", DEV, F32)
        return [t.detach() for t in outs] + [lv["opacity"].grad, lv["scaling"].grad]
    return run


def _sh_colors(P):
    def run(f):
        import test_sh_colors_gpu as T
        dev = [t.cuda() for t in T.make_inputs(P, 3, 3, 0)]
        return [T.kernel_route(3, *dev, split=False), T.kernel_route(2, *dev, split=True)]
    return run


def _sh_colors_views(P, V):
    def run(f):
        import test_sh_colors_views_gpu as T
        dc, rest, xyz, centres, cots, used = T.make_view_inputs(P, V, 3, 3)
        d = dict(dc=dc.cuda(), rest=rest.cuda(), xyz=xyz.cuda(), centres=[t.cuda() for t in centres], cots=[t.cuda() for t in cots], used=used)
        return [T.kernel_views(3, split=False, **d), T.kernel_views(3, split=True, **d)]
    return run


def _knn(P):
    def run(f):
        import knn_cases as KC
        from bags_raster.knn import distCUDA2
        return [distCUDA2(torch.tensor(KC.uniform(P, 5), device=DEV))]
    return run


def _lens(name):
    def run(f):
        import lens_cases as LC
        import test_lens_field_gpu as T
        from bags_raster.lens_field import lens_field_inverse
        c = LC.make_case(name)
        x = lens_field_inverse(c["params"].to(DEV), LC.inverse_input(name).to(DEV), *LC.dims(name), LC.INVERSE_ITERATIONS)
        return list(T._fused(name)) + [x]
    return run


def _resample(f):
    import test_resample_gpu as T
    H, W, h, w, fhw, chw = T.GEOM
    image, ctrl, cot = T._inputs(3, H, W, h, w, chw, 7)
    return list(T._hip(image, ctrl, fhw, chw, cot))


def _resample_faces(name):
    def run(f):
        import test_resample_faces_gpu as T
        return list(T._run(name))
    return run


# ------------------------------------------------------------------------------------------------------------------ cameras
def _camera_chain(f):
    import test_camera_gpu as T
    out = []
    for name in ("benign", "half_turn_x", "rotation_only", "scale_only"):        # both alignment inputs, neither, one of each
        d, cots = T._device_inputs(name)
        values, grads, _, _ = T._run(d, cots)
        out += [values, grads]
    return out


def _bank(n=18):
    import camera_cases as CC
    import test_pose_bank_gpu as T
    from bags_raster import PoseBank
    names = [k for k in CC.CASES]
    return PoseBank.from_cameras([T._case_camera(CC.make_case(names[i % len(names)])[0]) for i in range(n)], device=DEV)


def _pose_bank(f):
    """17 rows of a bank of 18, in reverse order: a second chunk of bags_pose_bank_forward / _backward, under a global alignment."""
    import camera_cases as CC
    bank = _bank()
    inp = CC.make_case("skewed_alignment")[0]
    gr = inp["grot"].to(F32).to(DEV).requires_grad_(True)
    gs = inp["gscale"].to(F32).to(DEV).requires_grad_(True)
    out = bank.get_matrices(list(range(17))[::-1], gr, gs)
    torch.autograd.backward(list(out), [torch.randn(o.shape, generator=_gen(60 + k)).to(DEV) for k, o in enumerate(out)])
    return [o.detach() for o in out] + [bank.leaves.grad, gr.grad, gs.grad]


def _pose_adam(f):
    from bags_raster import PoseAdam
    bank = _bank()
    opt = PoseAdam(bank, 1e-3, 1e-3, 1e-4)
    g = _gen(61)
    shape = tuple(bank.leaves.shape)
    bank.leaves.data = f.copy(bank.leaves.data)
    bank.leaves.grad = f.copy(torch.randn(shape, generator=g).to(DEV) * 0.01)
    opt.exp_avg, opt.exp_avg_sq = f.copy(torch.randn(shape, generator=g).to(DEV) * 0.01), f.copy(torch.rand(shape, generator=g).to(DEV) * 1e-4)
    opt.step(list(range(17))[::-1])
    opt.step([3, 17, 0], fov=False)
    return [bank.leaves.detach(), opt.exp_avg, opt.exp_avg_sq, opt.step_count]


# ------------------------------------------------------------------------------------------------------------------ in place
def _adam(P, stats):
    def run(f):
        import adam_reference as R
        import test_adam_gpu as T
        opt, params = T._ours(R.random_state(P, seed=P), step=4)
        _fence_optimizer(f, opt)
        kw, extra = {}, []
        if stats:
            g = _gen(3)
            radii = f.copy(torch.randint(-2, 40, (P,), generator=g).to(torch.int32).to(DEV))
            vsp = torch.zeros(P, 3, device=DEV, requires_grad=True)
            vsp.grad = f.copy(torch.randn(P, 3, generator=g).to(DEV))
            bag = SimpleNamespace(xyz_gradient_accum=f.copy(torch.rand(P, 1, generator=g).to(DEV)), denom=f.copy(torch.ones(P, 1).to(DEV)),
                                  max_radii2D=f.copy((torch.rand(P, generator=g) * 20).to(DEV)))
            kw = dict(visibility=radii, stats=(bag, vsp, radii))
            extra = [bag.xyz_gradient_accum, bag.denom, bag.max_radii2D]
        opt.step(**kw)
        return _opt_tensors(opt) + extra
    return run


def _densify(P):
    """densify_and_prune (bags_densify_plan + bags_densify_apply, whose outputs the wrapper allocates), then reset_opacity in place."""
    def run(f):
        import densify_reference as D
        import test_densify_gpu as T
        opt, bag, stats, noise = T._case(P, seed=11)
        _fence_optimizer(f, opt, bag)
        out = bag.densify_and_prune(opt, noise=noise[:, :2].contiguous().to(DEV), N=2, **D.RULE)
        res = [out["provenance"]] + [float(out[k]) for k in ("kept", "clones", "split", "pruned", "P_new")]
        res += [t.clone() if t is not None else None for t in _opt_tensors(opt)] + [bag.xyz_gradient_accum, bag.denom, bag.max_radii2D]
        _fence_optimizer(f, opt, bag)
        bag.reset_opacity(opt)
        return res + _opt_tensors(opt)
    return run


def _mcmc(P):
    """relocate (in place), add_new (new arrays from the wrapper), mcmc_noise (in place) and compute_relocation."""
    def run(f):
        import mcmc_reference as M
        import test_mcmc_gpu as T
        from bags_raster import compute_relocation, relocation_binoms
        opt, bag = T._case(P, 7, "GaussianAdam", 3, True)
        _fence_optimizer(f, opt, bag)
        mask = T._dead_patterns(P)["every_second"]
        dead, alive = mask.nonzero().reshape(-1).to(DEV), (~mask).nonzero().reshape(-1).to(DEV)
        res = [float(v) for v in bag.relocate(opt, mask.to(DEV), sampled=T._draw(bag, alive, int(dead.numel()), seed=P)).values()]
        res += [t.clone() if t is not None else None for t in _opt_tensors(opt)]
        A = int(1.05 * P) - P
        grown = bag.add_new(opt, 10 * P + 7, sampled=T._draw(bag, torch.arange(P, device=DEV), A, seed=P + 1))
        assert grown == {"added": A, "P_new": P + A}
        res += [t.clone() if t is not None else None for t in _opt_tensors(opt)] + [bag.xyz_gradient_accum, bag.denom, bag.max_radii2D]
        _fence_optimizer(f, opt, bag)
        bag.mcmc_noise(1e-3, noise=torch.randn(P + A, 3, generator=_gen(9)).to(DEV))
        o, s, N = M.relocation_inputs(P, P)
        return res + [bag._xyz.detach()] + list(compute_relocation(o.to(DEV), s.to(DEV), N.to(DEV), relocation_binoms(51, DEV), 51))
    return run


# ------------------------------------------------------------------------------------------------------------------ the table
class Row(SimpleNamespace):
    pass


def row(name, run, sizes=(), base=None, short=True, shapes="", why="", in_place=False):
    """``sizes``: the size functions of include/bags_raster.h whose buffers the row's calls are served from; ``base``: ROUNDED, GIVEN16
    or GIVEN4 -- what the header says of those buffers' base pointer (None: the row takes no workspace); ``short``: True -- every
    workspace call one byte short, the first refuses -- or ((call index, what the message names), ...); ``why``: the host-side
    allocations the row expects to pass through unfenced (none on the device ever may); ``in_place``: the entry point allocates
    nothing itself, the fenced tensors are the copies it is handed."""
    return Row(name=name, run=run, sizes=tuple(sizes), base=base, short=short if sizes else (), shapes=shapes, why=why, in_place=in_place)


HOST_CASE = "float64 host tensors of the case generator (torch.zeros_like of a permuted view), made when the case is first built"
STATE = ("bags_geom_size", "bags_image_size", "bags_binning_size", "bags_backward_workspace_size")
# Pinned words: _PinnedSlots.take allocates the host word a speculative forward's count arrives in with torch.zeros(1).pin_memory();
# the zeros are fenced, the pinned copy is made by torch.  Nothing passes through.
ROWS = [
    row("raster_auto", _raster(1000, 128, 96, 2.0, 3), STATE, ROUNDED, RASTER_SHORT, "P 1000, 128x96, degree 3, exact + speculative"),
    row("raster_radix", _raster(2000, 100, 70, 2.0, 0, binning="radix"), STATE, ROUNDED, RASTER_SHORT, "P 2000, 100x70, degree 0, binning radix"),
    row("raster_extras", _raster_extras, STATE, ROUNDED, ((3, "backward workspace"),), "P 1000, 128x96, depth and weights cotangents"),
    row("raster_empty", _raster_empty, STATE, ROUNDED, ((0, "geom buffer"), (1, "image buffer")), "P 0, 80x48, auto and radix"),
    row("speculative_overflow", _speculative(False), STATE, ROUNDED, (), "P 3000, 160x128, scales x 6 over the guess, default mode"),
    row("speculative_overflow_lazy", _speculative(True), STATE, ROUNDED, (), "the same with HOST_WAIT = lazy: SpeculationOverflow, then the retry"),
    row("render_views_normals", _render_step, STATE, ROUNDED, (), "5 PoseBank cameras, 72x40, render_views + render_normals"),
    row("factored_sh", _factored_sh, STATE, ROUNDED, (), "P 257, M 16, 2 views x 2 steps, bags_sh_gradient_from_views"),
    row("loss_scalar", _loss((3, 33, 31)), ("bags_loss_workspace_size",), GIVEN4, True, "(3,33,31)"),
    row("loss_vector", _loss((3, 40, 44)), ("bags_loss_workspace_size",), GIVEN4, True, "(3,40,44)"),
    row("camera_chain", _camera_chain, shapes="benign, half_turn_x, rotation_only, scale_only"),
    row("pose_bank", _pose_bank, shapes="17 rows of 18"),
    row("pose_adam", _pose_adam, shapes="17 rows of 18, then 3 without fov"),
    row("resample", _resample, ("bags_resample_workspace_size",), ROUNDED, True, "(3,33,47) -> (31,45)"),
    row("resample_faces_all", _resample_faces("all_faces"), ("bags_resample_faces_workspace_size",), ROUNDED, True, "all_faces"),
    row("resample_faces_hole", _resample_faces("hole"), ("bags_resample_faces_workspace_size",), ROUNDED, True, "hole"),
    row("activations", _activations(257, 3), shapes="P 257, degree 3"),
    row("activations_one", _activations(1, 2), shapes="P 1, degree 2"),
    row("activations_filtered", _activations_filtered(255), shapes="P 255"),
    row("gaussian_adam", _adam(257, False), shapes="P 257, six groups", in_place=True),
    row("gaussian_adam_stats", _adam(255, True), shapes="P 255, visibility + stats block", in_place=True),
    row("gaussian_adam_one", _adam(1, True), shapes="P 1, visibility + stats block", in_place=True),
    row("densify", _densify(257), ("bags_densify_workspace_size",), ROUNDED, True, "P 257, N 2, then reset_opacity"),
    row("densify_255", _densify(255), ("bags_densify_workspace_size",), ROUNDED, True, "P 255"),
    row("lens_field", _lens("b3_h33_n2_m257"), ("bags_lens_field_workspace_size",), ROUNDED, True, "b3_h33_n2_m257, forward backward inverse"),
    row("lens_field_one", _lens("b1_h1_n0_m1"), ("bags_lens_field_workspace_size",), ROUNDED, True, "b1_h1_n0_m1"),
    row("knn", _knn(257), ("bags_knn_workspace_size",), ROUNDED, True, "P 257"),
    row("knn_255", _knn(255), ("bags_knn_workspace_size",), ROUNDED, True, "P 255"),
    row("knn_one", _knn(1), ("bags_knn_workspace_size",), ROUNDED, True, "P 1"),
    row("mcmc", _mcmc(257), ("bags_mcmc_workspace_size",), ROUNDED, True, "P 257: relocate, add_new (+12), noise, compute_relocation"),
    row("mcmc_255", _mcmc(255), ("bags_mcmc_workspace_size",), ROUNDED, True, "P 255 (+12)"),
    row("antialias_255", _antialias(255), ("bags_antialias_workspace_size",), ROUNDED, True, "P 255"),
    row("antialias", _antialias(257), ("bags_antialias_workspace_size",), ROUNDED, True, "P 257, scale pair and cov3D"),
    row("antialias_one", _antialias(1), ("bags_antialias_workspace_size",), ROUNDED, True, "P 1"),
    row("filter3d", _filter3d(257), ("bags_filter3d_workspace_size",), ROUNDED, True, "P 257, 17 and 70 cameras"),
    row("filter3d_one", _filter3d(1), ("bags_filter3d_workspace_size",), ROUNDED, True, "P 1"),
    row("filter3d_255", _filter3d(255), ("bags_filter3d_workspace_size",), ROUNDED, True, "P 255"),
    row("appearance", _appearance, ("bags_appearance_workspace_size",), GIVEN16, True, "17x67, 17 views; stacked 3"),
    row("depth_prior_pearson", _depth_prior("pearson", "inverse"), ("bags_depth_prior_workspace_size",), GIVEN16, True, "17x67, 17 views"),
    row("depth_prior_l1", _depth_prior("l1", "depth"), ("bags_depth_prior_workspace_size",), GIVEN16, True, "17x67, 17 views, table"),
    row("normal_prior", _normal_prior, ("bags_normal_prior_workspace_size",), GIVEN16, True, "17x67 x 17 cos, 25x66 x 2 l1, depth_to_normal"),
    row("correspondence", _correspondence, ("bags_correspondence_workspace_size",), GIVEN16, True, "17x67, 17 pairs, reproject_pixels",
        why=HOST_CASE),
    row("warp", _warp, ("bags_warp_workspace_size",), GIVEN16, True, "17x67, 17 pairs, 3 channels, warp_image", why=HOST_CASE),
    row("bilagrid", _bilagrid, ("bags_bilagrid_workspace_size", "bags_bilagrid_tv_workspace_size"), GIVEN16, True, "grid 5x4x3, 21x67, 17 views; TV"),
    row("gaussian_normals", _gaussian_normals(257, 17), ("bags_gaussian_normals_workspace_size",), ROUNDED, True, "P 257, 17 views"),
    row("gaussian_normals_255", _gaussian_normals(255, 2), ("bags_gaussian_normals_workspace_size",), ROUNDED, True, "P 255, 2 views"),
    row("gaussian_normals_one", _gaussian_normals(1, 1), ("bags_gaussian_normals_workspace_size",), ROUNDED, True, "P 1, 1 view"),
    row("normal_map", _normal_map, ("bags_normal_map_workspace_size",), GIVEN16, True, "33x70 x 17, holes 33x70 x 5, 5x7 x 1"),
    row("depth_smooth", _smooth(False), ("bags_smooth_workspace_size",), GIVEN16, True, "33x70 x 17 twice, 5x7 x 1"),
    row("normal_smooth", _smooth(True), ("bags_smooth_workspace_size",), GIVEN16, True, "33x70 x 17 twice, 5x7 x 1"),
    row("gaussian_reg_257", _gaussian_reg(257), ("bags_gaussian_reg_workspace_size",), GIVEN16, True, "P 257, filtered + mask, plain"),
    row("gaussian_reg_255", _gaussian_reg(255), ("bags_gaussian_reg_workspace_size",), GIVEN16, True, "P 255"),
    row("gaussian_reg_one", _gaussian_reg(1), ("bags_gaussian_reg_workspace_size",), GIVEN16, True, "P 1"),
    row("sh_colors_257", _sh_colors(257), ("bags_sh_colors_workspace_size",), ROUNDED, True, "P 257, packed degree 3 and split degree 2"),
    row("sh_colors_255", _sh_colors(255), ("bags_sh_colors_workspace_size",), ROUNDED, True, "P 255"),
    row("sh_colors_one", _sh_colors(1), ("bags_sh_colors_workspace_size",), ROUNDED, True, "P 1"),
    row("sh_colors_views", _sh_colors_views(257, 16), ("bags_sh_colors_views_workspace_size",), ROUNDED, True, "P 257, 16 views"),
    row("sh_colors_views_5", _sh_colors_views(255, 5), ("bags_sh_colors_views_workspace_size",), ROUNDED, True, "P 255, 5 views, one unused"),
]
BY_NAME = {r.name: r for r in ROWS}
NAMES = [r.name for r in ROWS]


def test_every_size_function_of_the_header_is_in_a_row():
    """The 23 ``bags_*_workspace_size`` functions of _lib.SYMBOLS (= include/bags_raster.h; the backward's is one of them) and the
    three state buffers' size functions."""
    declared = {n for n in L.SYMBOLS if n.endswith("_workspace_size") or n in STATE}
    assert len(declared) == 26 and sum(n.endswith("_workspace_size") for n in declared) == 23, sorted(declared)
    covered = {s for r in ROWS for s in r.sizes}
    assert covered == declared, (sorted(declared - covered), sorted(covered - declared))


# ------------------------------------------------------------------------------------------------------------------ running a row
def _flat(x, out=None):
    """Every tensor of a nested result, on the host, in a fixed order; numbers and arrays as tensors, None kept as None."""
    out = [] if out is None else out
    if x is None or isinstance(x, str):
        out.append(None)
    elif isinstance(x, torch.Tensor):
        out.append(x.detach().cpu())
    elif isinstance(x, np.ndarray):
        out.append(torch.from_numpy(np.ascontiguousarray(x)))
    elif isinstance(x, (bool, int, float)):
        out.append(torch.tensor(float(x), dtype=torch.float64))
    elif isinstance(x, dict):
        for k in sorted(x):
            _flat(x[k], out)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _flat(v, out)
    else:
        raise TypeError("a row returned %r" % type(x))
    return out


@functools.lru_cache(maxsize=None)
def _plain(name):
    """The row in ordinary memory, once: shared by the tests, never written to."""
    res = BY_NAME[name].run(PLAIN)
    torch.cuda.synchronize()
    return _flat(res)


def _under(name, dirt, **kw):
    """The row under fences: (the fences, its results on the host -- gathered outside the block --, whether a result was fenced)."""
    with fenced(dirt, **kw) as f:
        res = BY_NAME[name].run(f)
        torch.cuda.synchronize()
    raw = []
    _tensors(res, raw)
    return f, _flat(res), any(f.is_fenced(t) for t in raw)


def _tensors(x, out):
    if isinstance(x, torch.Tensor):
        out.append(x)
    elif isinstance(x, dict):
        for v in x.values():
            _tensors(v, out)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _tensors(v, out)


@functools.lru_cache(maxsize=None)
def _fenced_run(name, dirt):
    return _under(name, dirt)


def _same(name, got, want, what):
    assert len(got) == len(want), (name, what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), (name, what, i)
        if a is None:
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, (name, what, i, a.shape, b.shape, a.dtype, b.dtype)
        # (bit equality, NaN included: a NaN a kernel computes is the same NaN every time; one read from 0xFF memory is not in `want`)
        same = torch.equal(a, b) or (a.is_floating_point() and torch.equal(torch.nan_to_num(a, nan=1.25e38), torch.nan_to_num(b, nan=1.25e38))
                                     and torch.equal(torch.isnan(a), torch.isnan(b)))
        assert same, "%s %s: tensor %d %s differs in %d of %d elements" % (name, what, i, tuple(a.shape), int((a != b).sum()), a.numel())


# ------------------------------------------------------------------------------------------------------------------ the helper on the device
def test_the_fences_work_on_the_device():
    """What tests/test_fenced_cpu.py holds on the host, on the GPU: 0xFF memory reads as NaN, a store one element past an output and
    one in front of it are seen (both land in bands this test owns), and an operation that forgets an element differs from its
    plain run under both dirts."""
    def forgetful(f):
        out = torch.empty(257, device=DEV)
        out[:256] = 1.0                                       # (element 256 is never written)
        return [out]
    with fenced(0xFF) as f:
        t = torch.empty(5, device=DEV)
        z = torch.zeros_like(t)
        ws = L.workspace(100, torch.device(DEV))
        got = _flat(forgetful(f))
    assert torch.isnan(t).all() and not z.any() and (ws == 0xFF).all() and f.is_fenced(t) and f.is_fenced(ws) and f.intact()
    assert t.data_ptr() % 512 == 0 and ws.data_ptr() % 512 == 0
    assert torch.isnan(got[0][256]) and (got[0][:256] == 1).all()
    with fenced(0xA5) as g:
        other = _flat(forgetful(g))
    assert not torch.equal(other[0], got[0]) and other[0][256] != 0
    torch.as_strided(t, (1,), (1,), t.storage_offset() + 5).fill_(1.0)
    torch.as_strided(ws, (1,), (1,), ws.storage_offset() - 1).fill_(0)
    assert not f.intact()
    rep = f.report()
    assert "(5,)" in rep and "after" in rep and "workspace #0 of 100 bytes" in rep and "before" in rep and rep.count("\n") == 1, rep


# ------------------------------------------------------------------------------------------------------------------ the properties
@pytest.mark.parametrize("dirt", DIRTS, ids=["a5", "ff"])
@pytest.mark.parametrize("name", NAMES)
def test_nothing_outside_is_written(name, dirt):
    f, _, _ = _fenced_run(name, dirt)
    assert f.intact(), f.report()


@pytest.mark.parametrize("name", NAMES)
def test_nothing_depends_on_what_the_memory_held(name):
    want = _plain(name)
    assert any(t is not None and t.numel() for t in want)
    for dirt in DIRTS:
        _same(name, _fenced_run(name, dirt)[1], want, "under 0x%02X against the plain run" % dirt)


@pytest.mark.parametrize("name", NAMES)
def test_the_interception_is_real(name):
    r = BY_NAME[name]
    f, _, any_fenced = _fenced_run(name, DIRTS[0])
    print("\nMEMORY_CONTRACT %-26s fenced %4d (by the package %4d)  workspaces %3d of %3d calls  skipped %d  a returned tensor fenced: %s"
          % (name, f.fenced, f.from_package, f.workspaces, f.workspace_calls, f.skipped, any_fenced))
    assert not f.skipped_on_device, f.skipped_on_device      # nothing the library can see passed through ...
    assert f.skipped == 0 or r.why, f.skipped_what           # ... and what did on the host is what the row says
    # the wrapper's own outputs, gradients or scratch came out fenced; an in-place entry point allocates nothing: its copies did
    assert f.from_package > 0 or (r.in_place and f.sites["copy"] > 0 and any_fenced), dict(f.sites)
    assert f.workspaces > 0 or not r.sizes


ROUNDED_ROWS = [r.name for r in ROWS if r.base == ROUNDED]
GIVEN_ROWS = [r.name for r in ROWS if r.base in (GIVEN16, GIVEN4)]
SHORT = [(r.name, which, what) for r in ROWS for which, what in (((None, "workspace"),) if r.short is True else r.short)]


@pytest.mark.parametrize("name", ROUNDED_ROWS)
def test_a_rounded_base_may_start_anywhere(name):
    """Every workspace call of the row starts one byte past a 512-byte boundary: rounding the base up uses the whole slack."""
    f, got, _ = _under(name, DIRTS[0], shift=1)
    assert f.workspaces > 0
    assert f.intact(), f.report()
    _same(name, got, _plain(name), "with every workspace shifted by 1 byte")


@pytest.mark.parametrize("name", GIVEN_ROWS)
def test_an_as_given_base_is_taken_at_its_alignment_and_refused_off_it(name):
    r = BY_NAME[name]
    for shift in (16,) if r.base == GIVEN16 else (16, 4):
        f, got, _ = _under(name, DIRTS[1], shift=shift)
        assert f.workspaces > 0
        assert f.intact(), f.report()
        _same(name, got, _plain(name), "with every workspace shifted by %d bytes" % shift)
    off = 4 if r.base == GIVEN16 else 1
    with fenced(DIRTS[0], shift=off) as f:
        with pytest.raises(RuntimeError, match="aligned"):
            r.run(f)
        torch.cuda.synchronize()
    assert f.workspaces > 0
    assert f.intact(), f.report()


@pytest.mark.parametrize("name,which,what", SHORT, ids=["%s-%s" % (n, "all" if w is None else w) for n, w, _ in SHORT])
def test_one_byte_short_is_refused(name, which, what):
    with fenced(DIRTS[0], shrink=1, which=which) as f:
        with pytest.raises(RuntimeError, match="workspace|" + what):
            BY_NAME[name].run(f)
        torch.cuda.synchronize()
    assert f.workspaces > 0 and (which is None or f.workspace_calls > which)
    assert f.intact(), f.report()
