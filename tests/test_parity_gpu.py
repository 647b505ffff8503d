"""-m gpu: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs.

Tolerances (BASELINE.json north_star): tile/splat indices bit-exact; gradients <= 1e-4 relative (L2 per tensor) to the
fp32 oracle and to the fp64 oracle replaying the fp32 run's discrete decisions; image |d| <= 1e-5 (1+|x|)."""
import pytest
import torch

from parity import (assert_ill_conditioned, assert_report, compare, compare_sampled, run_hip, run_oracle, sample_tiles,
                    tile_sort_paths)
from scenes import make_case, rel_err

pytestmark = pytest.mark.gpu


def _report(rep):
    import inspect
    from parity import dump_report
    print({k: v for k, v in rep.items()})
    dump_report(inspect.stack()[1].function, rep)


@pytest.mark.parametrize("P,W,H,sm,deg", [(1000, 128, 96, 2.0, 3), (3000, 200, 136, 1.5, 3), (2000, 100, 70, 2.0, 0),
                                          (4000, 160, 160, 1.0, 2), (2500, 131, 77, 2.0, 1)])
def test_parity_synthetic(P, W, H, sm, deg):
    scene, cam = make_case(P, W, H, sm, deg, seed=P)
    rep = compare(scene, cam, deg)
    _report(rep)
    assert_report(rep, skip_zero=("campos",) if deg == 0 else ())


def test_parity_config1_plumbing():
    """BASELINE config 1: 10k Gaussians, 400x400, SH degree 0."""
    scene, cam = make_case(10000, 400, 400, 1.0, 0, seed=0)
    rep = compare(scene, cam, 0, check_fp64=False, tile_bounds="aabb")
    _report(rep)
    assert rep["num_rendered"][0] == 270130          # SURVEY.md 8d (stock tile rule): G = 9 936, I = 0.27 M
    assert_report(rep, skip_zero=("campos",))
    rep = compare(scene, cam, 0, check_fp64=False)   # default: opacity-aware tile bounds
    assert rep["num_rendered"][0] == 138591
    assert_report(rep, skip_zero=("campos",))


def test_parity_background_and_scale_modifier():
    scene, cam = make_case(1500, 96, 64, 2.0, 3, seed=3)
    rep = compare(scene, cam, 3, bg=torch.tensor([0.3, 0.6, 0.9]), scale_modifier=0.7)
    _report(rep)
    assert_report(rep)


def test_parity_precomputed_colors_and_cov3D():
    scene, cam = make_case(1200, 96, 80, 2.0, 0, seed=5)
    g = torch.Generator().manual_seed(7)
    colors = torch.rand(1200, 3, generator=g)
    L = torch.randn(1200, 3, 3, generator=g) * 0.03
    cov = L @ L.transpose(1, 2)
    cov6 = torch.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1)
    rep = compare(scene, cam, 0, colors=colors, cov3D=cov6)
    _report(rep)
    assert_report(rep, skip_zero=("campos",))


def test_parity_shift_factors_extension():
    """Non-zero entrance-pupil polynomial (BASELINE config 5's distortion parameters).  theta = atan2(rho, z) is evaluated
    by the same libm-free operation sequence in the kernels and in the fp32 oracle (det_atan2_pos / _atan2_pos), so the
    integer artefacts are bit-exact with distortion switched on and values / gradients meet the ordinary bars."""
    scene, cam = make_case(1500, 128, 96, 2.0, 2, seed=9)
    rep = compare(scene, cam, 2, shift=torch.tensor([0.05, -0.02, 0.01]))
    _report(rep)
    assert_report(rep)
    scene, cam = make_case(20000, 400, 304, 1.0, 3, seed=10)
    # (the larger scene against the fp32 oracle alone: its fp64 replay was 40 s of the suite's CPU time, and config 5 at full size runs
    # with the distortion on as well)
    rep = compare(scene, cam, 3, shift=torch.tensor([-0.03, 0.02, 0.015]), check_fp64=False)
    _report({k: rep[k] for k in ("num_rendered", "image_max_err", "grad_rel_fp32")})
    assert_report(rep)


def test_frustum_clamp_gradient_semantic():
    """Decision D8.  Gaussians outside 1.3x the field of view get the clamped t.x = +-1.3 tanfovx t.z in the EWA Jacobian.
    DEFAULT (clamp_grad="stock"): upstream diff-gaussian-rasterization's backward, which the reference's fork inherits
    (README.md:126; op called at gaussian_renderer/__init__.py:110-121): dL/dt.x zeroed, the clamped t.x held constant inside
    dL/dt.z.  OPTION clamp_grad="exact": the clamped expression differentiated as written.  The camera sits inside the cloud
    with huge splats, so >100 clamped Gaussians reach the image: HIP must match the oracle of the SAME semantic to the
    ordinary bars in both modes, the two semantics must differ (on clamped Gaussians only), and forward values must not."""
    import math
    from scenes import camera_tensors
    P, W, H = 1200, 128, 96
    scene, cam = make_case(P, W, H, 5.0, 1, seed=5, dist=1.6)
    rep = compare(scene, cam, 1)                                   # default = stock, in the op and in the oracle
    _report({k: rep[k] for k in ("num_rendered", "image_max_err", "grad_rel_fp32", "grad_rel_fp64")})
    assert_report(rep, grad_tol=2e-4)
    rep_e = compare(scene, cam, 1, clamp_grad="exact")
    assert_report(rep_e, grad_tol=2e-4)
    g = torch.randn(3, H, W, generator=torch.Generator().manual_seed(1))
    outs_s, grads_s, _ = run_hip(scene, cam, 1, g)
    outs_e, grads_e, _ = run_hip(scene, cam, 1, g, clamp_grad="exact")
    assert all(torch.equal(a, b) for a, b in zip(outs_s, outs_e))   # the switch is a backward-only switch
    _, g_exact = run_oracle(scene, cam, 1, g, clamp_grad="exact")
    _, g_stock = run_oracle(scene, cam, 1, g)
    t = torch.cat([scene["means3D"], torch.ones(P, 1)], 1) @ camera_tensors(cam)["viewmatrix"]
    clamped = ((t[:, 0] / t[:, 2]).abs() > 1.3 * math.tan(cam.FoVx / 2)) | ((t[:, 1] / t[:, 2]).abs() > 1.3 * math.tan(cam.FoVy / 2))
    moved = (g_exact["means3D"] - g_stock["means3D"]).abs().sum(1) > 0
    assert int(moved.sum()) > 100 and not bool((moved & ~clamped).any())
    for k in ("means3D", "viewmatrix"):
        assert rel_err(grads_s[k], g_stock[k]) < 2e-4, (k, rel_err(grads_s[k], g_stock[k]))
        assert rel_err(grads_e[k], g_exact[k]) < 2e-4, (k, rel_err(grads_e[k], g_exact[k]))
        assert rel_err(grads_s[k], g_exact[k]) > 0.1, (k, rel_err(grads_s[k], g_exact[k]))
    # away from the clamp the two semantics are the same function: bit-identical gradients there
    assert torch.equal(grads_s["means3D"][~clamped], grads_e["means3D"][~clamped])


def test_edge_cases_empty_behind_and_single():
    from bags_raster.synth import look_at_origin_camera
    cam = look_at_origin_camera(64, 48)
    g = torch.randn(3, 48, 64, generator=torch.Generator().manual_seed(0))
    # everything behind the camera -> background only, zero gradients, I == 0
    scene, _ = make_case(50, 64, 48, 1.0, 1, seed=1)
    scene["means3D"] = scene["means3D"] + torch.tensor([0.0, 0.0, -10.0])
    bg = torch.tensor([0.2, 0.4, 0.6])
    outs, grads, views = run_hip(scene, cam, 1, g, bg=bg)
    assert views["num_rendered"] == 0 and int(outs[1].max()) == 0
    assert torch.allclose(outs[0], bg[:, None, None].expand(3, 48, 64))
    assert all(v is None or float(v.abs().max()) == 0.0 for v in grads.values())
    # a single Gaussian on the optical axis
    one = dict(means3D=torch.zeros(1, 3), scales=torch.full((1, 3), 0.2), rotations=torch.tensor([[1.0, 0, 0, 0]]),
               opacities=torch.tensor([[0.8]]), shs=torch.randn(1, 16, 3, generator=torch.Generator().manual_seed(2)) * 0.3)
    rep = compare(one, cam, 3)
    _report(rep)
    assert_report(rep)


def test_speculative_forward_of_a_scene_that_left_the_frustum():
    """Same problem shape, second call: a capacity hint exists, so the forward is speculative -- and this time NOTHING is in
    front of the camera (instance count 0: the emission launch runs on empty lists, no blend_bwd launch in the backward).
    Background only, zero gradients, and the next ordinary call is unaffected."""
    from bags_raster import rasterizer as R
    from bags_raster.synth import look_at_origin_camera
    cam = look_at_origin_camera(96, 80)
    g = torch.randn(3, 80, 96, generator=torch.Generator().manual_seed(3))
    scene, _ = make_case(400, 96, 80, 1.5, 1, seed=4)
    R._capacity_hint.clear()
    o1, g1, v1 = run_hip(scene, cam, 1, g)
    assert v1["num_rendered"] > 0 and R._capacity_hint
    gone = dict(scene); gone["means3D"] = scene["means3D"] + torch.tensor([0.0, 0.0, -20.0])
    bg = torch.tensor([0.1, 0.5, 0.9])
    o0, g0, v0 = run_hip(gone, cam, 1, g, bg=bg)
    assert v0["num_rendered"] == 0 and int(o0[1].max()) == 0
    assert torch.equal(o0[0], bg[:, None, None].expand(3, 80, 96).contiguous())
    assert all(v is None or float(v.abs().max()) == 0.0 for v in g0.values())
    o2, g2, _ = run_hip(scene, cam, 1, g)
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    for k in g1:
        if g1[k] is not None:
            assert torch.equal(g1[k], g2[k]), k


def test_saturated_alpha_and_early_termination():
    """Opaque, overlapping splats: exercises alpha clamp 0.99 and the T < 1e-4 stop."""
    scene, cam = make_case(800, 96, 96, 6.0, 1, seed=11)
    scene["opacities"] = torch.full_like(scene["opacities"], 0.999)
    rep = compare(scene, cam, 1)
    _report(rep)
    assert_report(rep, grad_tol=2e-4)


def test_depth_key_distance_mode():
    scene, cam = make_case(1500, 128, 96, 2.0, 1, seed=13)
    rep = compare(scene, cam, 1, depth_key="distance", check_fp64=False)
    _report(rep)
    assert_report(rep)


def test_backward_is_bitwise_reproducible():
    scene, cam = make_case(3000, 160, 128, 1.5, 3, seed=21)
    g = torch.randn(3, 128, 160, generator=torch.Generator().manual_seed(4))
    _, g1, _ = run_hip(scene, cam, 3, g)
    _, g2, _ = run_hip(scene, cam, 3, g)
    for k in g1:
        if g1[k] is not None:
            assert torch.equal(g1[k], g2[k]), k


def test_cpu_tensors_fail_loudly():
    from bags_raster import GaussianRasterizer
    from scenes import hip_settings
    scene, cam = make_case(10, 32, 32, 1.0, 0, seed=0)
    st = hip_settings(cam, 0, "cpu")
    with pytest.raises(RuntimeError, match="AMD GPU"):
        GaussianRasterizer(st)(means3D=scene["means3D"], means2D=torch.zeros(10, 3), shs=scene["shs"],
                               opacities=scene["opacities"], scales=scene["scales"], rotations=scene["rotations"])


def test_speculative_forward_matches_exact_and_recovers_from_overflow():
    """Second and later calls of a problem shape skip the mid-forward host round trip by guessing the instance capacity from
    earlier calls.  DEFAULT (HOST_WAIT = "forward"): the count is read before the forward returns and a too-small guess
    transparently redoes phase 2, so the image a forward returns is always the true render (train.py:250-331 computes its loss
    from it): a 6x jump of the instance count between two calls of one shape must return the ORACLE's image from forward
    itself, without any warning.  HOST_WAIT = "lazy" (opt-in): nothing in a training forward waits; results are identical
    whenever the guess holds; a guess that does not hold RAISES at backward entry (the loss came from an empty image) and the
    retried step is exact; with LAZY_RECOVER the state is recomputed instead (RuntimeWarning, exact gradients for the
    cotangent passed in); a lazy forward that is never differentiated reports the overflow when its count is collected."""
    import gc
    import warnings
    from bags_raster import rasterizer as R
    assert R.HOST_WAIT == "forward" and not R.LAZY_RECOVER, "the operator must be exact by default"
    scene, cam = make_case(3000, 160, 128, 1.0, 2, seed=31)
    g = torch.randn(3, 128, 160, generator=torch.Generator().manual_seed(5))
    big = dict(scene); big["scales"] = scene["scales"] * 6.0     # same shape, several times more instances than any guess
    saved = (R.HOST_WAIT, R.LAZY_RECOVER)

    def overflow_warnings(wlist):
        return [w for w in wlist if issubclass(w.category, RuntimeWarning) and "speculative capacity" in str(w.message)]
    try:
        # ---- default mode
        R._capacity_hint.clear()
        o_exact, g_exact, v1 = run_hip(scene, cam, 2, g)             # no hint yet: exact two-phase path
        assert R._capacity_hint, "hint not recorded"
        o_spec, g_spec, _ = run_hip(scene, cam, 2, g)                # hint present: speculative path
        for a, b in zip(o_exact, o_spec):
            assert torch.equal(a, b)
        for k in g_exact:
            if g_exact[k] is not None:
                assert torch.equal(g_exact[k], g_spec[k]), k
        with warnings.catch_warnings(record=True) as wlist:
            warnings.simplefilter("always")
            o_big, g_big, v_big = run_hip(big, cam, 2, g)            # the count jumps by more than 6x: forward redoes phase 2
        assert v_big["num_rendered"] > 6 * v1["num_rendered"], (v_big["num_rendered"], v1["num_rendered"])
        assert not overflow_warnings(wlist)
        st32, _ = run_oracle(big, cam, 2, None)
        err = ((o_big[0] - st32.image).abs() / (1.0 + st32.image.abs()))
        assert float((err > 1e-5).float().mean()) <= 2e-4 and float(err.max()) <= 5e-3, float(err.max())
        assert torch.equal(o_big[1], st32.radii)
        R._capacity_hint.clear()
        o_ref, g_ref, _ = run_hip(big, cam, 2, g)                    # exact path, no speculation
        for a, b in zip(o_big, o_ref):
            assert torch.equal(a, b)
        for k in g_ref:
            if g_ref[k] is not None:
                assert torch.equal(g_big[k], g_ref[k]), k
        # ---- lazy, opt-in: identical when the guess holds; raises on overflow; the retried step is exact
        R.HOST_WAIT = "lazy"
        R._capacity_hint.clear()
        run_hip(scene, cam, 2, g)
        o_lazy, g_lazy, _ = run_hip(scene, cam, 2, g)
        for a, b in zip(o_exact, o_lazy):
            assert torch.equal(a, b)
        for k in g_exact:
            if g_exact[k] is not None:
                assert torch.equal(g_exact[k], g_lazy[k]), k
        with pytest.raises(R.SpeculationOverflow):
            run_hip(big, cam, 2, g)
        o_retry, g_retry, _ = run_hip(big, cam, 2, g)                # the hint has been raised: fits now
        for a, b in zip(o_retry, o_ref):
            assert torch.equal(a, b)
        for k in g_ref:
            if g_ref[k] is not None:
                assert torch.equal(g_retry[k], g_ref[k]), k
        # ---- lazy with recovery
        R.LAZY_RECOVER = True
        R._capacity_hint.clear()
        run_hip(scene, cam, 2, g)
        with warnings.catch_warnings(record=True) as wlist:
            warnings.simplefilter("always")
            o_rec, g_rec, _ = run_hip(big, cam, 2, g)
        assert len(overflow_warnings(wlist)) == 1
        for a, b in zip(o_rec, o_ref):                               # the true image was written into the returned tensors
            assert torch.equal(a, b)
        for k in g_ref:
            if g_ref[k] is not None:
                assert torch.equal(g_rec[k], g_ref[k]), k
        R.LAZY_RECOVER = False
        # ---- lazy forward that is never differentiated: the overflow is reported when its count is collected
        R._capacity_hint.clear()
        run_hip(scene, cam, 2, g)
        from bags_raster import GaussianRasterizer
        from scenes import hip_settings
        dev = torch.device("cuda")
        t = {k: v.to(dev).requires_grad_(True) for k, v in big.items()}
        out = GaussianRasterizer(hip_settings(cam, 2, dev))(means3D=t["means3D"], means2D=torch.zeros(3000, 3, device=dev),
                                                             shs=t["shs"], opacities=t["opacities"], scales=t["scales"],
                                                             rotations=t["rotations"])
        torch.cuda.synchronize()
        del out
        gc.collect()
        with warnings.catch_warnings(record=True) as wlist:
            warnings.simplefilter("always")
            R._drain_abandoned()
        assert len(overflow_warnings(wlist)) == 1 and not R._abandoned
    finally:
        R.HOST_WAIT, R.LAZY_RECOVER = saved
        R._capacity_hint.clear()


@pytest.mark.timeout(900)
def test_full_size_config3_against_oracle():
    """BASELINE config 3 at full size (500 k Gaussians, 1920x1080, SH 3, pose + intrinsics learnable): integer artefacts
    bit-exact, image and EVERY gradient (Gaussian and pose) against the CPU oracle on all 8160 tiles.

    The 1e-4 bar is held against the fp32 oracle (the arithmetic of an fp32 reference rasterizer).  Against the fp64
    oracle -- even when it replays every fp32 threshold decision -- ANY fp32 rasterizer sits at 1e-4..1e-3: pixel
    centres near x = 1900 carry 1.2e-4 px of fp32 quantisation, which moves each Gaussian's gradient by ~1e-4
    relative; the fp32 oracle is exactly as far from fp64 as the HIP path is (printed: oracle32_vs_64).  shift_factors
    (an extension parameter, zero in the reference) is a sum of 5e5 terms of mixed sign and is only good to ~5e-3 in
    any fp32 evaluation."""
    import os
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    scene, cam = make_case(500_000, 1920, 1080, 0.5, 3, seed=0)
    rep = compare(scene, cam, 3, check_fp64=True)
    print({k: rep[k] for k in ("num_rendered", "n_contrib_mismatch_frac", "image_max_err", "image_bad_frac", "depth_max_err",
                               "weights_max_err", "mean2D_max_err", "grad_rel_fp32", "grad_rel_fp64", "oracle32_vs_64")})
    from parity import dump_report
    dump_report("test_full_size_config3_against_oracle", rep)
    # opacity-aware tile bounds (default); the stock 3-sigma rule gives 3 450 308 on this scene (~3.7 M)
    assert rep["num_rendered"][0] == rep["num_rendered"][1] == 2074322
    assert rep["n_contrib_mismatch_frac"] == 0.0, rep["n_contrib_mismatch_frac"]     # 2 073 600 pixels, every one identical
    # float outputs: TWO of the 2 073 600 pixels sit on a flipped threshold pair (a middle splat whose alpha lies within an ulp of
    # 1/255: the pixel's last contributor -- n_contrib, asserted identical above -- is not affected): image 2.8e-3 there, depth on
    # the same two pixels, weights on one (profiles/r05/parity_reports.jsonl); every other pixel is held to 1e-5 / 1e-4
    assert_report(rep, tol_override={"shift_factors": (1e-3, 1e-2)}, threshold_pixels=2)     # shift: measured 3.8e-4 vs fp32, 5.0e-3 vs fp64
    for k, e in rep["grad_rel_fp32"].items():
        if k != "shift_factors":
            assert e <= 1e-4, (k, e)
    # the HIP path must not be further from fp64 than the fp32 oracle itself is (x1.5 slack)
    for k, e in rep["grad_rel_fp64"].items():
        assert e <= 1.5 * rep["oracle32_vs_64"][k] + 1e-5, (k, e, rep["oracle32_vs_64"][k])


@pytest.mark.timeout(900)
def test_full_size_config3_aabb():
    """BASELINE config 3 at full size on the REFERENCE's instance list: tile_bounds="aabb" is the stock 3-sigma square the
    CUDA op behind gaussian_renderer/__init__.py:110-121 bins with (the second driver-timed leg of bench.py).  Integers
    bit-exact for all 500 k Gaussians and all 3 450 308 instances; image, n_contrib and every gradient on 96 sampled tiles
    (compare_sampled: the cotangent is zero outside them), fp32 oracle and fp64 replay."""
    import os
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    W, H = 1920, 1080
    scene, cam = make_case(500_000, W, H, 0.5, 3, seed=0)
    rep = compare_sampled(scene, cam, 3, sample_tiles(W, H, 96, seed=3), seed=2, check_fp64=True, tile_bounds="aabb")
    print({n: rep[n] for n in ("num_rendered", "instances_in_sample", "n_contrib_mismatch_frac", "image_max_err",
                               "image_bad_frac", "grad_rel_fp32", "grad_rel_fp64", "oracle32_vs_64")})
    from parity import dump_report
    dump_report("test_full_size_config3_aabb", rep)
    assert rep["num_rendered"][0] == rep["num_rendered"][1] == 3450308
    _assert_sampled(rep, skip=("shift_factors",))
    # shift_factors: identically zero parameter, a near-cancelling sum (see test_full_size_config3_against_oracle)
    assert min(rep["grad_rel_fp32"]["shift_factors"], rep["grad_rel_fp64"]["shift_factors"]) <= 1e-3


def _assert_sampled(rep, grad_tol=1e-4, worst_tol=2e-3, skip=(), nc_tol=0.0, threshold_pixels=0):
    """Bars of assert_report for a compare_sampled() report (the full-size configurations): integers bit-exact over ALL
    Gaussians / instances, n_contrib identical on the sampled pixels (nc_tol = 0 unless the caller says why not), image / depth /
    weights on EVERY sampled pixel (threshold_pixels = 0 unless the caller documents a pixel on a flipped threshold pair), every
    gradient <= grad_tol relative to the closer oracle (fp32 walk / fp64 replay)."""
    from parity import INT_KEYS, assert_image_bars
    for k in INT_KEYS:
        assert rep[k], f"{k} failed: {rep}"
    assert rep["num_rendered"][0] == rep["num_rendered"][1]
    assert rep["n_contrib_mismatch_frac"] <= nc_tol, rep["n_contrib_mismatch_frac"]
    assert_image_bars(rep, threshold_pixels, mean2D_tol=2e-3)
    g32, g64 = rep["grad_rel_fp32"], rep.get("grad_rel_fp64", rep["grad_rel_fp32"])
    for k in g32:
        if k in skip:
            continue
        best, worst = min(g32[k], g64.get(k, g32[k])), max(g32[k], g64.get(k, g32[k]))
        assert best <= grad_tol, f"grad[{k}]: best-of {best:.3e} > {grad_tol}: {rep}"
        assert worst <= worst_tol, f"grad[{k}]: worst-of {worst:.3e} > {worst_tol}: {rep}"
        if "oracle32_vs_64" in rep:      # never further from fp64 than the fp32 oracle itself is (x1.5 slack)
            assert g64[k] <= 1.5 * rep["oracle32_vs_64"][k] + 1e-5, (k, g64[k], rep["oracle32_vs_64"][k])


@pytest.mark.timeout(900)
def test_full_size_config4_views():
    """BASELINE config 4: 2 M Gaussians, three of the 200 perturbed-pose views (k = 0, 99, 199 of the radius-4 sphere,
    utils/pose_utils.py:59-64; so3 / translation noise 0.15 drawn with generator seed 55, scene/__init__.py:121-148) at
    1920x1080.  Integer artefacts bit-exact for all 2 M Gaussians and all ~6 M instances; image, n_contrib and every
    gradient against the oracle with the cotangent confined to 96 sampled tiles (compare_sampled)."""
    import os
    from bags_raster.synth import sphere_views, synth_scene
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    W, H = 1920, 1080
    scene = synth_scene(2_000_000, 0, 0.5, 3)
    cams = sphere_views(200, W, H, noise=0.15, seed=55)
    for k in (0, 99, 199):
        # the middle view on the REFERENCE's own instance list (tile_bounds="aabb": the stock 3-sigma square the CUDA op behind
        # gaussian_renderer/__init__.py:110-121 bins with), the other two on the default list
        tb = "aabb" if k == 99 else "opacity"
        rep = compare_sampled(scene, cams[k], 3, sample_tiles(W, H, 96, seed=k), seed=k + 1, check_fp64=True, tile_bounds=tb)
        print(k, tb, {n: rep[n] for n in ("num_rendered", "instances_in_sample", "n_contrib_mismatch_frac", "image_max_err",
                                      "image_bad_frac", "grad_rel_fp32", "grad_rel_fp64", "oracle32_vs_64")})
        from parity import dump_report
        dump_report(f"test_full_size_config4_views[k={k},{tb}]", rep)
        assert rep["num_rendered"][0] > (6_000_000 if tb == "aabb" else 3_000_000), rep["num_rendered"]
        # n_contrib: identical at k = 0 and k = 99; at k = 199 ONE of the 24 576 sampled pixels (4.1e-5) ends its list one splat
        # earlier or later than the oracle's -- a pair whose alpha sits within an ulp of 1/255 (the kernels evaluate exp as
        # exp2 of a pre-scaled power, torch's CPU exp is another implementation); the image agrees to 5e-7 there
        _assert_sampled(rep, nc_tol=0.0 if k != 199 else 1e-4)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("tile_bounds", ["opacity", "aabb"])
def test_full_size_config5_4k_with_distortion(tile_bounds):
    """BASELINE config 5 (on the default instance list and on the reference's own, tile_bounds="aabb"): 5 M Gaussians at 3840x2160, SH degree 3, NON-ZERO radial distortion parameters (the
    shift_factors polynomial, train.py:125,210-222; decision D2).  theta comes from the libm-free atan on both sides, so
    the integer artefacts stay bit-exact with distortion switched on: radii, rectangles, depth bits for all 5 M
    Gaussians, the sorted (key, id) list of all ~22 M instances, the 32 400 tile ranges.  Image, n_contrib and every
    gradient (incl. dL/dshift_factors) on 256 sampled tiles; the fp64 replay is added when the host has the memory."""
    import os
    from bags_raster.synth import look_at_origin_camera, synth_scene
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    W, H = 3840, 2160
    scene = synth_scene(5_000_000, 0, 0.5, 3)
    cam = look_at_origin_camera(W, H)
    sf = torch.tensor([0.02, -0.01, 0.005])
    try:
        import psutil
        big_host = psutil.virtual_memory().available > 48e9
    except ImportError:
        big_host = False
    rep = compare_sampled(scene, cam, 3, sample_tiles(W, H, 256, seed=5), seed=6, check_fp64=big_host, shift=sf, tile_bounds=tile_bounds)
    print({n: rep.get(n) for n in ("num_rendered", "instances_in_sample", "n_contrib_mismatch_frac", "image_max_err",
                                   "image_bad_frac", "grad_rel_fp32", "grad_rel_fp64", "oracle32_vs_64")})
    from parity import dump_report
    dump_report(f"test_full_size_config5_4k_with_distortion[{tile_bounds}]", rep)
    assert rep["num_rendered"][0] > (30_000_000 if tile_bounds == "aabb" else 15_000_000), rep["num_rendered"]
    # at 4K the fp32 pixel grid (ulp 2.4e-4 px at x = 3800) makes any fp32 rasterizer sit at ~1e-3 from fp64; without the
    # fp64 replay the bar against the fp32 oracle alone is 3e-4
    _assert_sampled(rep, grad_tol=1e-4 if big_host else 3e-4, nc_tol=1e-4)   # 65 536 sampled pixels; see config 4 for why not 0


def test_huge_splats_take_the_wave_cooperative_paths():
    """A few splats that cover most of the image (hundreds of tiles each): emission and per-Gaussian record summation
    switch to their wave-cooperative branches (> 32 / > 64 instances per Gaussian)."""
    scene, cam = make_case(150, 256, 192, 25.0, 1, seed=17)
    scene["opacities"] = scene["opacities"] * 0.5
    rep = compare(scene, cam, 1)
    _report({k: rep[k] for k in ("num_rendered", "image_max_err", "grad_rel_fp32", "grad_rel_fp64")})
    assert rep["num_rendered"][0] > 150 * 64, rep["num_rendered"]        # well past both thresholds on average
    assert_report(rep, grad_tol=2e-4)


def test_bundle_adjustment_recovers_a_perturbed_pose():
    """End-to-end use as in train.py (--opt_cam --opt_intrinsic): the four pose leaves of a camera (scene/cameras.py:99-110)
    are optimised with Adam (scene/__init__.py:164-193) through the op's viewmatrix / projmatrix / intrinsic / campos
    gradients and the photometric loss (train.py:311-325), Gaussians fixed.  The pose must move back towards the truth."""
    import math
    from bags_raster import GaussianRasterizationSettings, GaussianRasterizer
    from bags_raster.loss import photometric_loss
    from bags_raster.synth import look_at_origin_camera, synth_scene
    dev = torch.device("cuda")
    W, H = 160, 120
    scene = {k: v.to(dev) for k, v in synth_scene(4000, 3, 2.0, 2).items()}
    P = scene["means3D"].shape[0]

    def render(cam):
        st = GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
            bg=torch.zeros(3, device=dev), scale_modifier=1.0, viewmatrix=cam.get_world_view_transform(),
            projmatrix=cam.get_full_proj_transform(), intrinsic=cam.get_intrinsic(), sh_degree=2,
            campos=cam.get_camera_center(), prefiltered=False, debug=False, debug_iter=0)
        img, radii, depth, weights, mean2D = GaussianRasterizer(st)(
            means3D=scene["means3D"], means2D=torch.zeros(P, 3, device=dev), means2D_densify=torch.zeros(P, 3, device=dev),
            shift_factors=torch.zeros(3, device=dev), shs=scene["shs"], colors_precomp=None, opacities=scene["opacities"],
            scales=scene["scales"], rotations=scene["rotations"], cov3D_precomp=None)
        return img

    true_cam = look_at_origin_camera(W, H, device=dev)
    with torch.no_grad():
        target = render(true_cam)
    cam = look_at_origin_camera(W, H, device=dev)
    with torch.no_grad():
        cam.delta_translation += torch.tensor([[0.06], [-0.04], [0.08]], device=dev)
        cam.delta_quaternion += torch.tensor([0.0, 0.01, -0.012, 0.008], device=dev)
        cam.learnable_fovx += 0.02
    opt = torch.optim.Adam([{"params": [cam.delta_quaternion], "lr": 2e-3}, {"params": [cam.delta_translation], "lr": 5e-3},
                            {"params": [cam.learnable_fovx, cam.learnable_fovy], "lr": 2e-3}])

    def pose_err():
        return (cam.delta_translation.norm() + cam.delta_quaternion[1:].norm() + (cam.learnable_fovx - true_cam.FoVx).abs()).item()
    e0 = pose_err()
    losses = []
    for it in range(150):
        opt.zero_grad(set_to_none=True)
        loss = photometric_loss(render(cam), target)
        loss.backward()
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in cam.pose_leaves())
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < 0.35 * losses[0], (losses[0], losses[-1])
    assert pose_err() < 0.5 * e0, (e0, pose_err())


@pytest.mark.parametrize("case", ["tiny_scales", "huge_scales", "opaque_and_transparent", "near_plane", "off_screen", "needle"])
def test_extreme_inputs_match_oracle(case):
    """Degenerate / extreme Gaussians: sub-pixel splats (the 0.3 px dilation dominates), screen-filling splats,
    opacity 0 and ~1, points straddling the near plane, splats mostly off screen, extreme anisotropy."""
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
    rep = compare(scene, cam, 1, check_fp64=True)
    _report({k: rep[k] for k in ("num_rendered", "image_max_err", "image_bad_frac", "image_max_err_fp64",
                                 "oracle32_vs_64_image_max", "grad_rel_fp32", "grad_rel_fp64", "oracle32_vs_64")})
    if case == "needle":
        # 1500:1 anisotropy: fp32 itself is only good to ~1e-2 here (oracle fp32 vs fp64), so HIP is held to that
        assert_ill_conditioned(rep)
    else:
        assert_report(rep, grad_tol=3e-4, tol_override={"shift_factors": (1e-3, 1e-2)})


@pytest.mark.gpu
def test_render_caller_paths_agree_and_match_oracle():
    """render() (mirror of gaussian_renderer/__init__.py:30-133) assembles the op's arguments three ways -- rasterizer-side
    SH + scales/rotations, convert_SHs_python (eval_sh + 0.5, clamp), compute_cov3D_python (strip(L L^T)).  All three must
    render the same image and send the same gradients to the RAW leaves (pre-activation parameters and the four pose
    leaves of the camera), and the default path must match the oracle fed with the activated values."""
    from bags_raster.gaussians import GaussianBag
    from bags_raster.render import render, PipelineParams
    from bags_raster.synth import sphere_views
    dev = "cuda"
    P, W, H = 1500, 160, 128
    scene, _ = make_case(P, W, H, 1.5, 3, seed=17)
    cam = sphere_views(3, W, H, noise=0.05, device=dev)[2]
    cam0 = sphere_views(3, W, H, noise=0.05)[2]
    gimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(3)).to(dev)
    bgc = torch.tensor([0.2, 0.1, 0.3], device=dev)
    results = {}
    # "hybrid": the reference's own default (gaussian_renderer/__init__.py:30, hybrid=True): Python-side SH colours
    for name, pipe in (("default", PipelineParams()), ("sh_python", PipelineParams(convert_SHs_python=True)),
                       ("cov_python", PipelineParams(compute_cov3D_python=True)), ("hybrid", PipelineParams())):
        pc = GaussianBag.from_activated(scene, 3, device=dev)
        for p_ in cam.pose_leaves():
            p_.grad = None
        out = (render(cam, pc, pipe, bgc, 0.0, None, scaling_modifier=0.9) if name == "hybrid" else
               render(cam, pc, pipe, bgc, 0.0, None, hybrid=False, scaling_modifier=0.9))
        assert set(out) == {"render", "viewspace_points", "viewspace_points_densify", "visibility_filter", "radii", "depth",
                            "weights", "means2D"}
        out["render"].backward(gimg)
        assert out["viewspace_points"].grad is not None and out["viewspace_points_densify"].grad is not None
        assert torch.equal(out["visibility_filter"], out["radii"] > 0)
        results[name] = dict(img=out["render"].detach().cpu(), radii=out["radii"].cpu(),
                             leaves=[t.grad.detach().cpu().clone() for t in pc.leaves()],
                             pose=[t.grad.detach().cpu().clone() for t in cam.pose_leaves()],
                             vp=out["viewspace_points"].grad.detach().cpu(), vpd=out["viewspace_points_densify"].grad.detach().cpu())
    ref = results["default"]
    for name in ("sh_python", "cov_python", "hybrid"):
        r = results[name]
        assert torch.equal(r["radii"], ref["radii"])
        assert (r["img"] - ref["img"]).abs().max().item() < 2e-5, name
        for a, b in zip(r["leaves"] + r["pose"] + [r["vp"], r["vpd"]], ref["leaves"] + ref["pose"] + [ref["vp"], ref["vpd"]]):
            assert rel_err(a, b) < 2e-4, (name, rel_err(a, b))
    # default path against the oracle on activated values (same camera on the CPU)
    st32, gr32 = run_oracle(scene, cam0, 3, gimg.cpu(), torch.float32, bg=bgc.cpu(), scale_modifier=0.9)
    assert torch.equal(ref["radii"], st32.radii)
    assert ((ref["img"] - st32.image).abs() / (1 + st32.image.abs())).max().item() < 5e-5
    # chain the oracle's gradients w.r.t. activated values to the raw leaves with autograd on the CPU
    pc = GaussianBag.from_activated(scene, 3)
    acts = [pc.get_xyz, pc.get_features, pc.get_opacity, pc.get_scaling, pc.get_rotation]
    cots = [gr32["means3D"], gr32["shs"], gr32["opacities"], gr32["scales"], gr32["rotations"]]
    want = torch.autograd.grad(acts, pc.leaves(), cots)
    for a, b in zip(ref["leaves"], want):
        assert rel_err(a, b) < 3e-4, rel_err(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("P,W,H,sm,deg", [(3000, 200, 136, 1.5, 3), (2000, 100, 70, 2.0, 0)])
def test_parity_stock_aabb_tile_rule(P, W, H, sm, deg):
    """tile_bounds="aabb": the stock 3-sigma square of upstream 3DGS -- same bars as the default mode."""
    scene, cam = make_case(P, W, H, sm, deg, seed=P)
    rep = compare(scene, cam, deg, tile_bounds="aabb")
    _report(rep)
    assert_report(rep)


@pytest.mark.gpu
def test_tile_bound_modes_render_the_same():
    """Every (tile, Gaussian) pair the opacity-aware bounds drop has alpha < 1/255 on all 256 pixels, so the image, radii,
    depth and weights are bit-identical to the stock rule's and the gradients agree to summation order, with fewer
    sorted instances.  Includes low-opacity, saturated and strongly anisotropic splats."""
    scene, cam = make_case(6000, 320, 240, 1.5, 3, seed=77)
    g = torch.Generator().manual_seed(78)
    scene["opacities"] = torch.rand(6000, 1, generator=g) ** 3                     # many below 1/255, some near 1
    scene["scales"] = scene["scales"] * torch.exp(1.2 * torch.randn(6000, 3, generator=g))
    gimg = torch.randn(3, 240, 320, generator=g)
    o_t, g_t, v_t = run_hip(scene, cam, 3, gimg, tile_bounds="opacity")
    o_a, g_a, v_a = run_hip(scene, cam, 3, gimg, tile_bounds="aabb")
    assert v_t["num_rendered"] < 0.9 * v_a["num_rendered"], (v_t["num_rendered"], v_a["num_rendered"])
    for a, b in zip(o_t, o_a):                                                     # image, radii, depth, weights, mean2D
        assert torch.equal(a, b)
    for k in g_a:
        if g_a[k] is not None:
            # Only the order in which a Gaussian's per-tile records are added differs.  The screen-space sums agree to a few
            # ulps; behind the conic -> cov2D -> Sigma chain the strongly anisotropic splats of this scene amplify that.
            tol = 2e-6 if k in ("shs", "opacities", "means2D", "means2D_densify") else 1e-4
            assert rel_err(g_t[k], g_a[k]) < tol, (k, rel_err(g_t[k], g_a[k]))


@pytest.mark.gpu
@pytest.mark.timeout(600)
@pytest.mark.parametrize("P,W,H,shift", [(500_000, 1920, 1080, None), (5_000_000, 3840, 2160, (0.02, -0.01, 0.005))])
def test_tile_bound_modes_render_the_same_at_full_size(P, W, H, shift):
    """The headline runs on the default instance list (tile_bounds="opacity"), the reference's CUDA op on the stock 3-sigma list
    ("aabb", gaussian_renderer/__init__.py:110-121).  The claim that the one stands in for the other -- every pair the default rule
    drops has alpha < 1/255 on all 256 pixels of its tile -- is asserted HERE at BASELINE config 3 and config 5 size (with the
    distortion parameters on), not only on the 6 000-Gaussian scene above: image, radii, depth, weights, mean2D, n_contrib and
    final_T `torch.equal`; the gradients are the same sums in another order (a Gaussian's per-tile records: more of them, the
    extra ones zero).  No oracle involved: two runs of the product."""
    from bags_raster.synth import look_at_origin_camera, synth_scene
    scene, cam = synth_scene(P, 0, 0.5, 3), look_at_origin_camera(W, H)
    gimg = torch.randn(3, H, W, generator=torch.Generator().manual_seed(11))
    sf = None if shift is None else torch.tensor(shift)
    o_t, g_t, v_t = run_hip(scene, cam, 3, gimg, tile_bounds="opacity", shift=sf)
    o_a, g_a, v_a = run_hip(scene, cam, 3, gimg, tile_bounds="aabb", shift=sf)
    print({"instances": (v_t["num_rendered"], v_a["num_rendered"])})
    assert v_t["num_rendered"] < 0.7 * v_a["num_rendered"], (v_t["num_rendered"], v_a["num_rendered"])
    for name, a, b in zip(("image", "radii", "depth", "weights", "mean2D"), o_t, o_a):
        assert torch.equal(a, b), name
    assert torch.equal(v_t["n_contrib"] > 0, v_a["n_contrib"] > 0)          # (positions differ: they index two different lists)
    assert torch.equal(v_t["final_T"], v_a["final_T"])
    assert torch.equal(v_t["depth_bits"], v_a["depth_bits"])
    worst = {}
    for k in g_a:
        if g_a[k] is not None:
            worst[k] = rel_err(g_t[k], g_a[k])
            # summation order only.  shift_factors: a near-cancelling sum over all Gaussians (test_full_size_config3_against_oracle)
            assert worst[k] < (2e-3 if k == "shift_factors" else 2e-5), (k, worst[k])
    print(worst)


@pytest.mark.gpu
@pytest.mark.parametrize("binning", ["auto", "radix"])
def test_tile_masks_on_slanted_needles(binning):
    """D7, second half: needle-shaped splats at random angles, 40 to 160 px long -- rectangles on both sides of the 8 x 8
    tile limit of the masks, most of whose tiles the ellipse never reaches.  The lists (both binning paths) are the
    oracle's bit for bit, well under half of the rectangles' tiles are emitted, and the image is the stock rule's, bit
    for bit."""
    P, W, H = 2500, 512, 384
    scene, cam = make_case(P, W, H, 1.0, 2, seed=91)
    g = torch.Generator().manual_seed(92)
    length = torch.exp(torch.empty(P, 1).uniform_(-2.6, -1.2, generator=g))          # world units; ~40..160 px on screen
    scene["scales"] = torch.cat([length, length / 40.0, length / 40.0], 1)[:, torch.randperm(3, generator=g)]
    q = torch.randn(P, 4, generator=g)
    scene["rotations"] = q / q.norm(dim=1, keepdim=True)
    scene["opacities"] = torch.rand(P, 1, generator=g) * 0.9 + 0.05
    rep = compare(scene, cam, 2, check_fp64=False, binning=binning)
    _report({k: rep[k] for k in ("num_rendered", "tiles_touched_equal", "point_list_equal", "ranges_equal", "image_max_err")})
    # needles are ill conditioned in fp32 (a conic entry of 3 times an offset of 100 px, squared): the value bars of the
    # ordinary scenes do not apply (tests of their own: test_needle_*); here the integer artefacts and the masks are the point
    from parity import INT_KEYS
    for k in INT_KEYS:
        assert rep[k], k
    assert rep["num_rendered"][0] == rep["num_rendered"][1] == 49715
    assert rep["n_contrib_mismatch_frac"] <= 1e-3 and rep["image_max_err"] <= 5e-3 and rep["image_bad_frac"] <= 2e-3
    gimg = torch.randn(3, H, W, generator=g)
    o_t, _, v_t = run_hip(scene, cam, 2, gimg, tile_bounds="opacity", binning=binning)
    o_a, _, v_a = run_hip(scene, cam, 2, gimg, tile_bounds="aabb", binning=binning)
    rect = v_t["rect"].long()
    w_, h_ = rect[:, 2] - rect[:, 0], rect[:, 3] - rect[:, 1]
    vis = o_t[1] > 0                                                                   # radii
    assert int(((w_ > 8) | (h_ > 8))[vis].sum()) > 20 and int(((w_ <= 8) & (h_ <= 8) & (w_ * h_ > 16))[vis].sum()) > 200
    small = vis & (w_ <= 8) & (h_ <= 8)
    kept, area = int(v_t["tiles_touched"][small].sum()), int((w_ * h_)[small].sum())
    assert kept < 0.6 * area, (kept, area)                                            # slanted needles: most of the box is empty
    large = vis & ~small
    assert torch.equal(v_t["tiles_touched"][large].long(), (w_ * h_)[large])          # larger rectangles emit every tile
    for a, b in zip(o_t, o_a):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_means2D_offsets_and_debug_mode_match_oracle():
    """Non-zero additive NDC offsets in means2D (decision D4) move the splats and receive gradient; debug=True (a sync and an
    error check after every kernel, pipe.debug in the reference) must not change any result."""
    scene, cam = make_case(1500, 144, 112, 2.0, 1, seed=21)
    off = torch.zeros(1500, 3)
    off[:, :2] = 0.02 * torch.randn(1500, 2, generator=torch.Generator().manual_seed(5))
    rep = compare(scene, cam, 1, means2D=off)
    _report({k: rep[k] for k in ("num_rendered", "image_max_err", "grad_rel_fp32")})
    assert_report(rep)
    g = torch.randn(3, 112, 144, generator=torch.Generator().manual_seed(6))
    o0, g0, _ = run_hip(scene, cam, 1, g, means2D=off)
    o1, g1, _ = run_hip(scene, cam, 1, g, means2D=off, debug=True)
    for a, b in zip(o0, o1):
        assert torch.equal(a, b)
    for k in g0:
        if g0[k] is not None:
            assert torch.equal(g0[k], g1[k]), k


@pytest.mark.gpu
def test_debug_mode_names_the_tensor_that_went_non_finite():
    """debug=True (pipe.debug, gaussian_renderer/__init__.py:63): besides the sync + error check after every kernel, the op
    scans what it produced for NaN / Inf and raises naming the tensor and the iteration; without debug nothing is scanned."""
    from bags_raster import GaussianRasterizer
    from scenes import hip_settings
    scene, cam = make_case(800, 96, 80, 2.0, 1, seed=3)
    dev = torch.device("cuda")
    bad = {k: v.to(dev).clone() for k, v in scene.items()}
    bad["shs"][::7, 0, 1] = float("inf")                                     # a poisoned colour (NaN would be clamped away by max(0, .)): reaches the image
    kw = dict(means3D=bad["means3D"], means2D=torch.zeros(800, 3, device=dev), shs=bad["shs"], opacities=bad["opacities"],
              scales=bad["scales"], rotations=bad["rotations"])
    out = GaussianRasterizer(hip_settings(cam, 1, dev))(**kw)                # no debug: no scan, the Infs simply come out
    assert not bool(torch.isfinite(out[0]).all())
    with pytest.raises(RuntimeError, match="non-finite values in rendered_image at iteration 0"):
        GaussianRasterizer(hip_settings(cam, 1, dev, debug=True))(**kw)
    # a clean forward whose cotangent is poisoned: the backward scan names a gradient
    good = {k: v.to(dev).clone().requires_grad_(True) for k, v in scene.items()}
    img = GaussianRasterizer(hip_settings(cam, 1, dev, debug=True))(
        means3D=good["means3D"], means2D=torch.zeros(800, 3, device=dev), shs=good["shs"], opacities=good["opacities"],
        scales=good["scales"], rotations=good["rotations"])[0]
    cot = torch.ones_like(img)
    cot[:, 40, 48] = float("inf")
    with pytest.raises(RuntimeError, match="the backward produced .* non-finite values in grad_"):
        img.backward(cot)


@pytest.mark.gpu
def test_side_stream_and_non_contiguous_inputs():
    """The library enqueues on torch's CURRENT stream, and the shim accepts non-contiguous views (gradients flow back to
    the original tensors): results are bitwise those of the default-stream, contiguous call."""
    from bags_raster import GaussianRasterizer
    from scenes import hip_settings
    dev = torch.device("cuda")
    scene, cam = make_case(1200, 128, 96, 2.0, 3, seed=23)
    cot = torch.randn(3, 96, 128, generator=torch.Generator().manual_seed(7)).to(dev)

    def run(stream, strided):
        t = {k: v.to(dev).clone() for k, v in scene.items()}
        if strided:       # scales as every second column of a wider tensor, rotations as a transposed-back view
            wide = torch.zeros(1200, 6, device=dev); wide[:, ::2] = t["scales"]; wide.requires_grad_(True)
            rot_src = t["rotations"].t().contiguous().requires_grad_(True)
            scales, rots = wide[:, ::2], rot_src.t()
            leaves = dict(scales=wide, rotations=rot_src)
        else:
            scales, rots = t["scales"].requires_grad_(True), t["rotations"].requires_grad_(True)
            leaves = dict(scales=scales, rotations=rots)
        m3 = t["means3D"].requires_grad_(True)
        ctx = torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream())
        with ctx:
            st = hip_settings(cam, 3, dev)
            out = GaussianRasterizer(st)(means3D=m3, means2D=torch.zeros(1200, 3, device=dev), means2D_densify=torch.zeros(1200, 3, device=dev),
                                         shift_factors=torch.zeros(3, device=dev), shs=t["shs"], colors_precomp=None,
                                         opacities=t["opacities"], scales=scales, rotations=rots, cov3D_precomp=None)
            out[0].backward(cot)
        torch.cuda.synchronize()
        gs = leaves["scales"].grad
        gr = leaves["rotations"].grad
        if strided:
            assert (gs[:, 1::2] == 0).all()
            gs, gr = gs[:, ::2].contiguous(), gr.t().contiguous()
        return out[0].detach().clone(), m3.grad.clone(), gs.clone(), gr.clone()
    base = run(None, False)
    side = run(torch.cuda.Stream(), False)
    strided = run(None, True)
    for a, b, c in zip(base, side, strided):
        assert torch.equal(a, b) and torch.equal(a, c)


@pytest.mark.parametrize("P,W,H,sm,deg", [(3000, 200, 136, 1.5, 3), (150, 256, 192, 25.0, 1)])
def test_binning_paths_give_identical_lists(P, W, H, sm, deg):
    """binning="auto" (tile-binned: count matrix + per-tile LDS sort, csrc/binning.hip) and binning="radix" (depth sort of
    the Gaussians + stable radix sort of the instances, csrc/sort.hip) must produce the same sorted lists, tile ranges,
    outputs and gradients bit for bit -- and the radix path stays held to the oracle."""
    scene, cam = make_case(P, W, H, sm, deg, seed=P)
    if P == 150:
        scene["opacities"] = scene["opacities"] * 0.5
    g = torch.randn(3, H, W, generator=torch.Generator().manual_seed(2))
    o_a, g_a, v_a = run_hip(scene, cam, deg, g, binning="auto")
    o_r, g_r, v_r = run_hip(scene, cam, deg, g, binning="radix")
    assert v_a["num_rendered"] == v_r["num_rendered"] > 0
    for k in ("point_list", "keys_sorted", "n_contrib", "tiles_touched", "rect"):
        assert torch.equal(v_a[k], v_r[k]), k
    nz = (v_r["ranges"][:, 1] - v_r["ranges"][:, 0]) > 0
    assert torch.equal(v_a["ranges"][nz], v_r["ranges"][nz])
    assert torch.equal(v_a["ranges"][:, 1] - v_a["ranges"][:, 0], v_r["ranges"][:, 1] - v_r["ranges"][:, 0])
    for a, b in zip(o_a, o_r):
        assert torch.equal(a, b)
    for k in g_a:
        if g_a[k] is not None:
            assert torch.equal(g_a[k], g_r[k]), k
    rep = compare(scene, cam, deg, binning="radix", check_fp64=False)
    assert_report(rep, grad_tol=2e-4)


def test_binning_paths_agree_on_random_scenes():
    """Randomised cross-check of the two list builders (no oracle: fast): odd image sizes, 1 .. 60 k Gaussians, mixed
    anisotropy and opacity, both tile rules, both depth keys -- lists, ranges, outputs and gradients must be bit-identical
    (gradients with the stock tile rule: to summation order, see below)."""
    rng = torch.Generator().manual_seed(2024)
    for trial in range(14):
        P = int(torch.randint(1, 60000, (1,), generator=rng)) if trial else 1
        W = int(torch.randint(17, 700, (1,), generator=rng)); H = int(torch.randint(17, 500, (1,), generator=rng))
        sm = float(torch.empty(1).uniform_(0.3, 4.0, generator=rng))
        deg = int(torch.randint(0, 4, (1,), generator=rng))
        scene, cam = make_case(P, W, H, sm, deg, seed=1000 + trial)
        if trial % 3 == 1:                                   # needles
            scene["scales"] = scene["scales"] * torch.exp(1.5 * torch.randn(P, 3, generator=rng))
        if trial % 4 == 2:
            scene["opacities"] = torch.rand(P, 1, generator=rng) ** 3
        kw = dict(tile_bounds="aabb" if trial % 5 == 3 else "opacity", depth_key="distance" if trial % 2 else "z")
        g = torch.randn(3, H, W, generator=rng)
        o_a, g_a, v_a = run_hip(scene, cam, deg, g, binning="auto", **kw)
        o_r, g_r, v_r = run_hip(scene, cam, deg, g, binning="radix", **kw)
        tag = (trial, P, W, H, round(sm, 2), deg, kw)
        assert v_a["num_rendered"] == v_r["num_rendered"], tag
        for k in ("point_list", "keys_sorted", "n_contrib", "tiles_touched", "rect"):
            assert torch.equal(v_a[k], v_r[k]), (k, tag)
        assert torch.equal(v_a["ranges"][:, 1] - v_a["ranges"][:, 0], v_r["ranges"][:, 1] - v_r["ranges"][:, 0]), tag
        for a, b in zip(o_a, o_r):
            assert torch.equal(a, b), tag
        for k in g_a:
            if g_a[k] is not None:
                if kw["tile_bounds"] == "opacity":
                    assert torch.equal(g_a[k], g_r[k]), (k, tag)
                else:
                    # stock tile rule: the tile-binned path keeps gradient records only for the tiles the opacity rule reaches
                    # (the others are exact zeros on the radix path), so a Gaussian with more than 64 records has them dealt to
                    # the lanes of its wave-cooperative sum differently: equal to summation order, not bit for bit
                    # (and the backward's chunks hold other splats: compacted record holders against consecutive list positions).
                    # Measured: <= 2.2e-6; 8e-4 for dL/dscales of the needle scenes, whose sums cancel by four digits (fp32 itself
                    # is good to ~1e-2 there: test_extreme_inputs_match_oracle[needle])
                    assert rel_err(g_a[k], g_r[k]) <= (3e-3 if trial % 3 == 1 else 2e-5), (k, tag, rel_err(g_a[k], g_r[k]))


@pytest.mark.parametrize("P,shrink,flat", [(3000, 0.04, False), (20000, 0.02, False), (40000, 0.012, False),
                                           (600, 0.3, True), (2500, 0.03, True), (5000, 0.03, True)])
def test_long_and_clustered_tile_lists_take_every_sort_path(P, shrink, flat):
    """The per-tile sort of the tile-binned path (csrc/binning.hip) has four ways through it; each must give the oracle's list:
    thousands of splats over a handful of tiles (a camera far from a compact scene) leave the one-wave bucket sort for the
    workgroup-wide one (513..2048 entries) or the two-level slab sort (P = 3000, 20000 and 40000: 2049..65536 entries; the
    global-memory network above that has its own test, test_tile_sort_limit_of_the_slab_path); `flat` puts every splat at the SAME depth (identical 32-bit keys: the order is decided by the
    Gaussian id alone), which overflows the buckets / slabs and takes the bitonic fallbacks (in LDS for P = 600 and 2500, in
    global memory for P = 5000)."""
    scene, cam = make_case(P, 64, 48, 1.0, 0, seed=P + 1)
    scene["means3D"] = scene["means3D"] * shrink
    if flat:
        scene["means3D"][:, 2] = 0.25
    scene["opacities"] = scene["opacities"] * (0.05 if not flat else 0.2)      # keep the pixels from saturating
    rep = compare(scene, cam, 0, check_fp64=False)
    _report({k: rep[k] for k in ("num_rendered", "image_max_err", "n_contrib_mismatch_frac", "grad_rel_fp32")})
    out, _, views = run_hip(scene, cam, 0)
    longest = int((views["ranges"][:, 1] - views["ranges"][:, 0]).max())
    if flat:
        vis = views["depth_bits"][out[1] > 0]
        assert vis.numel() > 100 and int((vis != vis[0]).sum()) == 0, "depth keys are not identical"
    else:
        assert longest > {3000: 1024, 20000: 8192, 40000: 16384}[P], longest
    assert_report(rep, grad_tol=3e-4, skip_zero=("campos",))


@pytest.mark.parametrize("N", [255, 256, 257, 510, 511, 512, 513, 2047, 2048, 2049])
def test_tile_sort_size_boundaries(N):
    """One tile holding exactly N instances, N on either side of every size at which the per-tile sort changes its code path
    (csrc/binning.hip: half-size one-wave instance <= 256, one wave <= 512, whole workgroup <= 2048, slabs above): the list must
    be the radix path's, bit for bit (no oracle: fast)."""
    scene, cam = make_case(N, 48, 48, 1.0, 0, seed=N)
    gen = torch.Generator().manual_seed(N)
    xyz = 0.004 * torch.randn(N, 3, generator=gen)          # all of them project into the middle of tile (1, 1)
    xyz[:, 2] = torch.rand(N, generator=gen) - 0.5          # depths spread out: distinct keys, arbitrary order
    scene["means3D"] = xyz
    scene["scales"] = torch.full((N, 3), 0.003)
    scene["opacities"] = torch.full((N, 1), 0.05)
    g = torch.randn(3, 48, 48, generator=gen)
    o_a, g_a, v_a = run_hip(scene, cam, 0, g, binning="auto")
    o_r, g_r, v_r = run_hip(scene, cam, 0, g, binning="radix")
    lens = v_r["ranges"][:, 1] - v_r["ranges"][:, 0]
    assert int(lens.max()) == N and int((lens > 0).sum()) == 1, lens
    assert v_a["num_rendered"] == v_r["num_rendered"] == N
    for k in ("point_list", "keys_sorted", "n_contrib"):
        assert torch.equal(v_a[k], v_r[k]), k
    for a, b in zip(o_a, o_r):
        assert torch.equal(a, b)
    for k in g_a:
        if g_a[k] is not None:
            assert torch.equal(g_a[k], g_r[k]), k
    if N < 600:     # ... and against the oracle where the forward's chunks end (255 staged splats per chunk: 255 | 256, 510 | 511)
        rep = compare(scene, cam, 0, check_fp64=False)
        _report({k: rep[k] for k in ("num_rendered", "image_max_err", "n_contrib_mismatch_frac", "grad_rel_fp32")})
        assert_report(rep, grad_tol=3e-4, skip_zero=("campos",))


@pytest.mark.parametrize("N,bands", [(2304, (0, 2, 4, 6, 8)), (2304, (0, 1, 7, 8)), (5000, (0, 3, 4, 9, 10, 15, 19))])
def test_slab_sort_with_empty_and_single_entry_slabs(N, bands):
    """The two-level sort of a 2049..65536-entry list cuts the depth-key range into K = min(256, ceil(N / 256)) equal slabs and lets the
    four waves draw them from a counter.  Depth-clustered lists leave slabs EMPTY or with ONE entry: a wave that drew such a slab
    used to leave the list altogether (`return` for `continue`, csrc/tile_sort.h), and with enough of them no wave was left
    for the last slabs -- their part of the sorted list kept whatever the buffer held before (tools/soak.py: a memory fault
    once a camera had drifted into the scene).  One tile, depths in bands that populate only the slabs in ``bands`` plus a
    lone entry in an otherwise empty slab; the list must be the radix path's, bit for bit."""
    scene, cam = make_case(N, 48, 48, 1.0, 0, seed=N)
    gen = torch.Generator().manual_seed(N + len(bands))
    K = (N + 255) // 256
    xyz = 0.004 * torch.randn(N, 3, generator=gen)          # all of them project into the middle of tile (1, 1)
    # view depth = z + 4 in [4, 4 + span]: inside one binade, so the float bits -- the sort key -- are linear in it
    span = 1.8
    w = span / K
    which = torch.tensor(bands)[torch.randint(0, len(bands), (N,), generator=gen)]
    z = (which.float() + 0.1 + 0.8 * torch.rand(N, generator=gen)) * w
    lone = [k for k in range(K) if k not in bands][0]
    z[0], z[1], z[2] = 0.0, span * (1 - 1e-6), (lone + 0.5) * w          # first key, last key, the lone entry
    xyz[:, 2] = z
    scene["means3D"] = xyz
    scene["scales"] = torch.full((N, 3), 0.003)
    scene["opacities"] = torch.full((N, 1), 0.02)
    g = torch.randn(3, 48, 48, generator=gen)
    o_r, g_r, v_r = run_hip(scene, cam, 0, g, binning="radix")
    lens = v_r["ranges"][:, 1] - v_r["ranges"][:, 0]
    assert int(lens.max()) == N and int((lens > 0).sum()) == 1, lens
    for attempt in range(3):                                # which wave draws which slab varies from run to run
        o_a, g_a, v_a = run_hip(scene, cam, 0, g, binning="auto")
        assert v_a["num_rendered"] == v_r["num_rendered"] == N
        for k in ("point_list", "keys_sorted", "n_contrib"):
            assert torch.equal(v_a[k], v_r[k]), (k, attempt)
        for a, b in zip(o_a, o_r):
            assert torch.equal(a, b)
        for k in g_a:
            if g_a[k] is not None:
                assert torch.equal(g_a[k], g_r[k]), k


def test_dense_scene_against_oracle(monkeypatch):
    """A dense scene: sm 3.0, thousands of instances per tile (the longest list well above 3000: the two-level slab sort), every
    pixel saturated long before its list ends, so that most instances lie behind their tile's deepest contributor.  The backward
    then runs in dense-scene mode (a byte per gradient record; blend_bwd writes no zero records, preprocess_bwd reads none:
    BagsBackwardArgs.dense_per_tile).  Lists, ranges and n_contrib bit-exact against the oracle, gradients to the ordinary bars --
    and bit-identical between the two modes of the backward (the records one of them skips are the zeros of the other)."""
    from bags_raster import rasterizer as R
    scene, cam = make_case(20000, 128, 96, 3.0, 2, seed=33)
    monkeypatch.setattr(R, "DENSE_PER_TILE", 0)               # library default: on for this scene
    rep = compare(scene, cam, 2, check_fp64=False)
    _report({k: rep[k] for k in ("num_rendered", "image_max_err", "n_contrib_mismatch_frac", "grad_rel_fp32")})
    assert rep["num_rendered"][0] > 600 * 48, rep["num_rendered"]          # above the default threshold of the dense mode
    assert_report(rep, grad_tol=2e-4)
    g = torch.randn(3, 96, 128, generator=torch.Generator().manual_seed(4))
    o_d, g_d, v_d = run_hip(scene, cam, 2, g)
    lens = v_d["ranges"][:, 1] - v_d["ranges"][:, 0]
    assert int(lens.max()) >= 3000, int(lens.max())
    took = tile_sort_paths(v_d["keys_sorted"], v_d["ranges"])
    assert any(k.startswith("slabs") for k in took), took
    per_pixel_len = lens.view(6, 8)[torch.arange(96)[:, None] // 16, torch.arange(128)[None, :] // 16]
    assert float((v_d["n_contrib"] < per_pixel_len // 2).float().mean()) > 0.8       # the walks end in the first half of their lists (0.89)
    monkeypatch.setattr(R, "DENSE_PER_TILE", -1)              # never: zero records written and read
    o_z, g_z, v_z = run_hip(scene, cam, 2, g)
    for a, b in zip(o_d, o_z):
        assert torch.equal(a, b)
    for k in g_d:
        if g_d[k] is not None:
            assert torch.equal(g_d[k], g_z[k]), k


@pytest.mark.parametrize("tile_bounds", ["opacity", "aabb"])
def test_wide_chunks_that_overflow_a_wave_copy(tile_bounds):
    """The backward stages 224 (240 on sparse scenes) splats per chunk and keeps, per wave, 176 (168) slots for the ones that reach the
    wave's quadrant (blend.hip, BCHUNK / BSLOTS, WCHUNK / WSLOTS; 8 slots fewer with the stock tile rule, whose chunks are staged
    from the compacted lists); a chunk in which more splats than that reach some quadrant runs its group phase twice, once per half.
    A scene of huge, faint splats on a 4 x 3-tile image: ~400 instances in every tile, every splat reaching every quadrant, walks
    that go deep into the lists -- every full chunk overflows.  Against the oracle to the ordinary bars, with both tile rules; the host
    re-derives that the case is what it claims."""
    import numpy as np
    from oracle import raster_oracle as O
    from scenes import oracle_settings
    from parity import chunk_quadrant_counts
    scene, cam = make_case(420, 64, 48, 8.0, 1, seed=21)
    scene["opacities"] = scene["opacities"] * 0.2
    rep = compare(scene, cam, 1, tile_bounds=tile_bounds)
    _report({k: rep[k] for k in ("num_rendered", "image_max_err", "n_contrib_mismatch_frac", "grad_rel_fp32", "grad_rel_fp64")})
    assert_report(rep)
    T = 12
    assert rep["num_rendered"][0] > 300 * T, rep["num_rendered"]
    g = torch.randn(3, 48, 64, generator=torch.Generator().manual_seed(1))
    _, g_b, v = run_hip(scene, cam, 1, g, tile_bounds=tile_bounds)
    _, g_r, v_r = run_hip(scene, cam, 1, g, tile_bounds=tile_bounds, binning="radix")       # the radix path's lists feed the same backward
    assert torch.equal(v["point_list"], v_r["point_list"])
    for k in g_b:                           # (stock tile rule: the tile-binned path stages its chunks from the compacted lists, the radix path
        if g_b[k] is not None:              # from the full ones -- other chunk boundaries, other scan groups: equal to rounding, not to the bit)
            assert torch.equal(g_b[k], g_r[k]) if tile_bounds == "opacity" else rel_err(g_b[k], g_r[k]) < 1e-5, k
    s = oracle_settings(cam, 1, tile_bounds=tile_bounds)
    P = scene["means3D"].shape[0]
    with torch.no_grad():
        pre = O.preprocess(scene["means3D"], torch.zeros(P, 3), torch.zeros(3), scene["shs"], None, scene["opacities"], scene["scales"],
                           scene["rotations"], None, s, torch.float32, None)
    xy, conic, op = pre.xy.numpy().astype(np.float64), pre.conic.numpy().astype(np.float64), pre.opacity.numpy().astype(np.float64)
    # (at least) the first, deepest chunk of either geometry: 224 consecutive list positions from the tile's deepest contributor
    chunks = chunk_quadrant_counts(v["point_list"].numpy(), v["ranges"].numpy(), v["n_contrib"].numpy(), xy, conic, op, 4, 224)
    overflowing = sum(bool(c) and c[0][1] > 176 for c in chunks.values())
    two_chunks = sum(sum(n for n, _ in c) > 240 for c in chunks.values())
    assert len(chunks) == T and overflowing >= 6 and two_chunks >= 3, (overflowing, two_chunks)


def test_conic_backward_semantic():
    """Decision D9.  DEFAULT conic_grad="stock": upstream computeCov2DCUDA's backward of the 2x2 inverse divides by det^2 + 1e-7
    (the reference's fork inherits it, README.md:126); "exact" divides by det^2 (rounds 1-4).  A scene of small splats (det near
    its floor of 0.09, where the regulariser weighs most): each mode against the oracle of the SAME mode to the ordinary bars,
    forward outputs bit-identical between the modes, the gradients of the two modes apart by more than rounding and by less than
    the 1.2e-5 ceiling."""
    scene, cam = make_case(4000, 160, 96, 0.25, 1, seed=9)
    g = torch.randn(3, 96, 160, generator=torch.Generator().manual_seed(2))
    res = {}
    for mode in ("stock", "exact"):
        rep = compare(scene, cam, 1, conic_grad=mode)
        _report({k: rep[k] for k in ("num_rendered", "image_max_err", "grad_rel_fp32", "grad_rel_fp64")})
        assert_report(rep)
        res[mode] = run_hip(scene, cam, 1, g, conic_grad=mode)
    for a, b in zip(res["stock"][0], res["exact"][0]):
        assert torch.equal(a, b)
    for k in ("means3D", "scales", "rotations"):
        e = rel_err(res["stock"][1][k], res["exact"][1][k])
        assert 1e-9 < e < 1.3e-5, (k, e)
    for k in ("shs", "opacities", "means2D"):                   # nothing downstream of the conic
        assert torch.equal(res["stock"][1][k], res["exact"][1][k]), k


def _oracle_lists(scene, cam, deg, **kw):
    """The oracle's instance list alone (preprocess + binning; no blending): sorted ids, 64-bit keys, tile ranges."""
    from oracle import raster_oracle as O
    from scenes import oracle_settings
    s = oracle_settings(cam, deg, **kw)
    P = scene["means3D"].shape[0]
    with torch.no_grad():
        pre = O.preprocess(scene["means3D"], torch.zeros(P, 3), torch.zeros(3), scene["shs"], None, scene["opacities"], scene["scales"],
                           scene["rotations"], None, s, torch.float32, None)
        gx, gy = (cam.image_width + 15) // 16, (cam.image_height + 15) // 16
        keys, pl, ranges, _ = O.bin_and_sort(pre.depth.float(), pre.rect, pre.tiles_touched, gx, gy, pre.keep)
    return keys, pl, ranges


@pytest.mark.parametrize("N", [65535, 65536, 65537])
@pytest.mark.parametrize("depths", ["spread", "banded", "flat"])
def test_tile_sort_limit_of_the_slab_path(N, depths):
    """ONE tile holding exactly N instances, N on either side of TSORT_LARGE = 65536 (csrc/tile_sort.h): up to there the two-level
    slab sort (256 slabs of ~256 entries, a wave per slab), above it the bitonic network in global memory -- the limit was
    16384 until the end of round 4 and no test stood at the new one.  `spread`: depths uniform, every slab ~256 entries (slabs
    at 65535 / 65536, network at 65537); `banded`: three quarters of the slabs populated, the others empty (the shape that lost
    entries in rounds 3-4); `flat`: one identical depth, i.e. one slab that outgrows a wave -> the network on both sides.  The
    list must be the radix path's AND the oracle's, bit for bit; image, n_contrib and gradients the radix path's."""
    scene, cam = make_case(N, 48, 48, 1.0, 0, seed=N)
    gen = torch.Generator().manual_seed(N + len(depths))
    xyz = 0.004 * torch.randn(N, 3, generator=gen)          # all of them project into the middle of tile (1, 1)
    span = 1.8                                              # view depth = z + 4 in [4, 5.8]: one binade, keys linear in depth
    if depths == "spread":
        z = span * torch.rand(N, generator=gen)
    elif depths == "banded":
        K = 256
        r = torch.randint(0, 3 * K // 4, (N,), generator=gen)
        band = r + r // 3                                   # slabs 3, 7, 11, ... stay empty, the others hold ~341 entries
        z = (band.float() + 0.1 + 0.8 * torch.rand(N, generator=gen)) * (span / K)
        z[0], z[1] = 0.0, span * (1 - 1e-6)                 # first and last key pin the slab grid
    else:
        z = torch.full((N,), 0.25)
    xyz[:, 2] = z
    scene["means3D"] = xyz
    scene["scales"] = torch.full((N, 3), 0.003)
    scene["opacities"] = torch.full((N, 1), 0.02)
    g = torch.randn(3, 48, 48, generator=gen)
    o_r, g_r, v_r = run_hip(scene, cam, 0, g, binning="radix")
    lens = v_r["ranges"][:, 1] - v_r["ranges"][:, 0]
    assert int(lens.max()) == N and int((lens > 0).sum()) == 1, lens
    took = tile_sort_paths(v_r["keys_sorted"], v_r["ranges"])
    want = "network" if (N > 65536 or depths == "flat") else "slabs"
    assert list(took) == [want], (took, want)               # the side of the limit this case is meant to stand on
    o_a, g_a, v_a = run_hip(scene, cam, 0, g, binning="auto")
    assert v_a["num_rendered"] == v_r["num_rendered"] == N
    for k in ("point_list", "keys_sorted", "n_contrib"):
        assert torch.equal(v_a[k], v_r[k]), k
    for a, b in zip(o_a, o_r):
        assert torch.equal(a, b)
    for k in g_a:
        if g_a[k] is not None:
            assert torch.equal(g_a[k], g_r[k]), k
    keys, pl, ranges = _oracle_lists(scene, cam, 0)
    assert torch.equal(v_a["point_list"], pl) and torch.equal(v_a["keys_sorted"], keys)
    nz = ranges[:, 1] > ranges[:, 0]
    assert torch.equal(v_a["ranges"][nz], ranges[nz])


@pytest.mark.parametrize("tile_bounds", ["opacity", "aabb"])
def test_frozen_camera_mode_against_oracle(tile_bounds):
    """The op as the reference calls it without --opt_cam / --opt_intrinsic (train.py:472-485 steps the camera leaves only under
    those flags; BASELINE config 2, "fixed pose"): camera tensors without a gradient, means2D_densify = None, shift_factors =
    None, i.e. NULL for grad_viewmatrix .. grad_campos, grad_means2D_densify (the backward instantiated without the abs sums)
    and grad_shift_factors (gaussian_renderer/__init__.py:110-121 passes the same keywords).  Until round 5 this mode was timed
    and compared with itself only.  Every Gaussian gradient against the oracle, and against the op's own full mode."""
    scene, cam = make_case(3000, 200, 136, 1.5, 3, seed=3000)
    rep = compare(scene, cam, 3, frozen_camera=True, tile_bounds=tile_bounds)
    _report({k: rep[k] for k in ("num_rendered", "image_max_err", "n_contrib_mismatch_frac", "grad_rel_fp32", "grad_rel_fp64")})
    assert set(rep["grad_rel_fp32"]) == {"means3D", "means2D", "shs", "opacities", "scales", "rotations"}, rep["grad_rel_fp32"].keys()
    assert_report(rep)
    g = torch.randn(3, 136, 200, generator=torch.Generator().manual_seed(1))
    o_f, g_f, _ = run_hip(scene, cam, 3, g, frozen_camera=True, tile_bounds=tile_bounds)
    o_p, g_p, _ = run_hip(scene, cam, 3, g, tile_bounds=tile_bounds)
    for a, b in zip(o_f, o_p):
        assert torch.equal(a, b)
    for k in ("viewmatrix", "projmatrix", "intrinsic", "campos", "means2D_densify", "shift_factors"):
        assert g_f[k] is None, k
    for k in ("means3D", "means2D", "shs", "opacities", "scales", "rotations"):
        assert rel_err(g_f[k], g_p[k]) <= 1e-6, (k, rel_err(g_f[k], g_p[k]))     # the same sums with and without the pose Jacobians beside them


@pytest.mark.parametrize("tile_bounds", ["opacity", "aabb"])
def test_frozen_camera_mode_at_config2_size(tile_bounds):
    """BASELINE config 2 itself: 500 k Gaussians, 1920x1080, SH degree 3, fixed pose -- on the default instance list and on the
    reference's own (tile_bounds="aabb").  Integers bit-exact for all Gaussians and instances, image / n_contrib / Gaussian
    gradients on 96 sampled tiles (the cotangent is zero elsewhere)."""
    scene, cam = make_case(500_000, 1920, 1080, 0.5, 3, seed=0)
    rep = compare_sampled(scene, cam, 3, sample_tiles(1920, 1080, 96, seed=7), frozen_camera=True, tile_bounds=tile_bounds)
    _report({n: rep[n] for n in ("num_rendered", "instances_in_sample", "n_contrib_mismatch_frac", "image_max_err", "grad_rel_fp32")})
    from parity import dump_report
    dump_report(f"test_frozen_camera_mode_at_config2_size[{tile_bounds}]", rep)
    assert rep["num_rendered"][0] == (3_450_308 if tile_bounds == "aabb" else 2_074_322)
    assert set(rep["grad_rel_fp32"]) == {"means3D", "means2D", "shs", "opacities", "scales", "rotations"}
    _assert_sampled(rep)


@pytest.mark.parametrize("W,H,P,sm,shrink,fovy", [
    (10, 7, 200, 3.0, 1.0, None),            # less than one tile
    (16, 2000, 1500, 0.2, 1.0, None),        # one column of 125 tiles
    (2100, 48, 1500, 0.3, 1.0, 0.0313),      # three rows of 132 tiles: more than one run of 128 descriptors (fovx = 1.2 rad)
    (530, 270, 2500, 1.5, 0.25, None)])      # scene in the image centre: most of the 578 tiles are empty
def test_tile_list_shapes(W, H, P, sm, shrink, fovy):
    """Both blend launches take their tiles from the heavy-first descriptor list (tile_order_kernel): every tile must be
    rendered exactly once whatever the tile count (below, at and above multiples of the 128-descriptor runs) and however
    many tiles are empty (they come last in the list; the backward skips them)."""
    kw = {} if fovy is None else dict(fovy=fovy)
    scene, cam = make_case(P, W, H, sm, 2, seed=W + H, **kw)
    scene["means3D"] = scene["means3D"] * shrink
    rep = compare(scene, cam, 2, check_fp64=False)
    _report(rep)
    assert rep["num_rendered"][0] > 0
    assert_report(rep)


@pytest.mark.gpu
def test_two_views_in_flight_on_two_streams():
    """Two views of one problem shape rendered concurrently on two streams (what a multi-view batch does): each call has its
    own pinned word for the asynchronous instance count and its own state buffers, so both must reproduce, bit for bit, what
    they give when run one after the other on the default stream."""
    from bags_raster import GaussianRasterizer
    from bags_raster.synth import sphere_views
    from scenes import hip_settings
    dev = torch.device("cuda")
    scene, _ = make_case(6000, 256, 192, 1.2, 3, seed=51)
    cams = sphere_views(4, 256, 192, noise=0.05)[2:4]
    cot = torch.randn(3, 192, 256, generator=torch.Generator().manual_seed(9)).to(dev)
    base = {k: v.to(dev) for k, v in scene.items()}

    def run(cam, stream):
        t = {k: v.clone().requires_grad_(True) for k, v in base.items()}
        with torch.cuda.stream(stream):
            st = hip_settings(cam, 3, dev)
            out = GaussianRasterizer(st)(means3D=t["means3D"], means2D=torch.zeros(6000, 3, device=dev), means2D_densify=torch.zeros(6000, 3, device=dev),
                                         shift_factors=torch.zeros(3, device=dev), shs=t["shs"], colors_precomp=None, opacities=t["opacities"],
                                         scales=t["scales"], rotations=t["rotations"], cov3D_precomp=None)
            out[0].backward(cot)
        return out, t
    cur = torch.cuda.current_stream()
    ref = []
    for c in cams:                                            # twice each: the second call of a shape takes the speculative path
        run(c, cur); o, t = run(c, cur)
        torch.cuda.synchronize()
        ref.append((o[0].detach().clone(), o[1].clone(), {k: v.grad.clone() for k, v in t.items()}))
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    sa.wait_stream(cur); sb.wait_stream(cur)
    for rep in range(3):
        oa, ta = run(cams[0], sa)
        ob, tb = run(cams[1], sb)
        torch.cuda.synchronize()
        for (o, t), r in (((oa, ta), ref[0]), ((ob, tb), ref[1])):
            assert torch.equal(o[0].detach(), r[0]) and torch.equal(o[1], r[1])
            for k in r[2]:
                assert torch.equal(t[k].grad, r[2][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(2560, 1440), (1936, 1088), (130, 1000)])
def test_tile_counts_of_every_ranges_order_variant(W, H):
    """The single-workgroup ranges / tile-order kernel is instantiated for 8, 16 and 32 tiles per thread (the last two
    with more than 64 KB of dynamic LDS); 14 400 tiles (2560x1440) take the middle one, 8228 (one row past 1080p) the first
    tile count above 8192, 567 a narrow image where most threads own no tile.  Lists bit-exact over all tiles, blending
    on a sample."""
    scene, cam = make_case(20000, W, H, 0.5, 1, seed=W)
    rep = compare_sampled(scene, cam, 1, sample_tiles(W, H, 32, seed=2))
    print({k: rep[k] for k in ("num_rendered", "instances_in_sample", "image_max_err")})
    assert rep["num_rendered"][0] > 20_000
    _assert_sampled(rep, grad_tol=2e-4)


@pytest.mark.gpu
def test_exactly_32768_tiles_stay_on_the_tile_binned_path():
    """4096x2048 = 32 768 tiles, the largest image the tile-binned path takes: tile_count_kernel then asks for 65 536 B of
    dynamic LDS next to its 64 B of static LDS, which needs the explicit opt-in above 64 KB (the launch failed with
    BAGS_ERR_HIP without it).  Lists bit-exact against the oracle AND identical to the radix path's."""
    W, H = 4096, 2048
    scene, cam = make_case(4000, W, H, 0.25, 1, seed=5)
    rep = compare_sampled(scene, cam, 1, sample_tiles(W, H, 32, seed=4))
    print({k: rep[k] for k in ("num_rendered", "instances_in_sample", "image_max_err", "grad_rel_fp32")})
    assert rep["num_rendered"][0] > 50_000
    _assert_sampled(rep, grad_tol=2e-4)
    _, _, va = run_hip(scene, cam, 1, binning="auto")
    _, _, vr = run_hip(scene, cam, 1, binning="radix")
    assert torch.equal(va["point_list"], vr["point_list"]) and torch.equal(va["keys_sorted"], vr["keys_sorted"])


@pytest.mark.gpu
def test_more_than_32768_tiles_falls_back_to_the_radix_path():
    """34 170 tiles (3216x2720): beyond the tile-binned path's LDS limits, so binning="auto" must take the radix path by
    itself -- same bit-exact lists; blending checked on 48 sampled tiles."""
    scene, cam = make_case(3000, 3216, 2720, 0.25, 1, seed=3)
    rep = compare_sampled(scene, cam, 1, sample_tiles(3216, 2720, 48, seed=1))
    print({k: rep[k] for k in ("num_rendered", "instances_in_sample", "image_max_err", "grad_rel_fp32")})
    assert rep["num_rendered"][0] > 100_000
    _assert_sampled(rep, grad_tol=2e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("binning", ["auto", "radix"])
def test_zero_gaussians_render_the_background(binning):
    """P = 0 (a scene pruned to nothing): no prepare phase runs at all; the forward must still produce the background, the
    backward zeros for the camera tensors."""
    from bags_raster import GaussianRasterizer
    from bags_raster.synth import look_at_origin_camera
    from scenes import camera_tensors, hip_settings
    dev = torch.device("cuda")
    cam = look_at_origin_camera(80, 48)
    ct = {k: v.clone().requires_grad_(True) for k, v in camera_tensors(cam, dev).items()}
    bg = torch.tensor([0.1, 0.5, 0.9])
    st = hip_settings(cam, 2, dev, bg=bg, tensors=ct, binning=binning)
    z = lambda *s: torch.zeros(*s, device=dev)
    out = GaussianRasterizer(st)(means3D=z(0, 3), means2D=z(0, 3), means2D_densify=z(0, 3), shift_factors=z(3), shs=z(0, 9, 3),
                                 colors_precomp=None, opacities=z(0, 1), scales=z(0, 3), rotations=z(0, 4), cov3D_precomp=None)
    assert out[0].shape == (3, 48, 80) and out[1].numel() == 0
    assert torch.allclose(out[0].cpu(), bg[:, None, None].expand(3, 48, 80))
    out[0].sum().backward()
    for k, v in ct.items():
        assert v.grad is None or float(v.grad.abs().max()) == 0.0, k


@pytest.mark.parametrize("M,deg,P", [(16, 3, 3001), (16, 1, 700), (4, 1, 515), (9, 2, 130)])
def test_split_sh_pair_equals_the_concatenated_tensor(M, deg, P):
    """ABI 7: shs = features_dc (P,1,3) + shs_rest = features_rest (P,M-1,3), the reference's two parameters as they are stored
    (scene/gaussian_model.py:131-134), against the same values concatenated: image, radii and every other gradient bit for bit,
    the two feature gradients = the two slices of dL/dshs -- M = 16 goes through the staged whole-line stores (tail float4 of
    an odd P included), other M through the per-row form; active degree below the stored one; then once more accumulating."""
    from bags_raster import GaussianRasterizer
    from bags_raster import rasterizer as R
    from scenes import hip_settings
    dev = torch.device("cuda", 0)
    scene, cam = make_case(P, 176, 112, 1.5, 3, seed=5)
    shs = scene["shs"][:, :M, :].contiguous()
    rast = GaussianRasterizer(hip_settings(cam, deg, dev))
    g = torch.randn(3, 112, 176, generator=torch.Generator().manual_seed(9)).to(dev)

    def run(split, leaves=None, accumulate=False):
        if leaves is None:
            base = {k: scene[k].to(dev).clone().requires_grad_(True) for k in ("means3D", "opacities", "scales", "rotations")}
            if split:
                base["dc"] = shs[:, :1, :].contiguous().to(dev).requires_grad_(True)
                base["rest"] = shs[:, 1:, :].contiguous().to(dev).requires_grad_(True)
            else:
                base["shs"] = shs.to(dev).clone().requires_grad_(True)
            leaves = base
        m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
        kw = dict(shs=leaves["dc"], shs_rest=leaves["rest"]) if split else dict(shs=leaves["shs"])
        R.ACCUMULATE_IN_PLACE = accumulate
        try:
            out = rast(means3D=leaves["means3D"], means2D=m2d, means2D_densify=None, shift_factors=None, colors_precomp=None,
                       opacities=leaves["opacities"], scales=leaves["scales"], rotations=leaves["rotations"], cov3D_precomp=None, **kw)
            out[0].backward(g)
        finally:
            R.ACCUMULATE_IN_PLACE = False
        return out, leaves, m2d
    o0, l0, m0 = run(False)
    o1, l1, m1 = run(True)
    assert torch.equal(o0[0], o1[0]) and torch.equal(o0[1], o1[1])
    for k in ("means3D", "opacities", "scales", "rotations"):
        assert torch.equal(l0[k].grad, l1[k].grad), k
    assert torch.equal(m0.grad, m1.grad)
    assert l1["dc"].grad.shape == (P, 1, 3) and l1["rest"].grad.shape == (P, M - 1, 3)
    assert torch.equal(l1["dc"].grad, l0["shs"].grad[:, :1, :]) and torch.equal(l1["rest"].grad, l0["shs"].grad[:, 1:, :])
    if deg < 3 and (deg + 1) ** 2 < M:
        assert float(l1["rest"].grad[:, (deg + 1) ** 2 - 1:, :].abs().max()) == 0.0          # inactive coefficients: exact zeros
    # a second view accumulating in place into the pair's .grad (the view-sharded step, sharding.py)
    first = {k: v.grad.clone() for k, v in l1.items()}
    run(True, l1, accumulate=True)
    for k, v in l1.items():
        assert torch.allclose(v.grad, 2.0 * first[k], rtol=1e-6, atol=1e-7), k
    # only one of the pair wanted
    dc = shs[:, :1, :].contiguous().to(dev); rest = shs[:, 1:, :].contiguous().to(dev).requires_grad_(True)
    out = rast(means3D=l0["means3D"].detach(), means2D=None, means2D_densify=None, shift_factors=None, colors_precomp=None,
               opacities=l0["opacities"].detach(), scales=l0["scales"].detach(), rotations=l0["rotations"].detach(),
               cov3D_precomp=None, shs=dc, shs_rest=rest)
    out[0].backward(g)
    assert torch.equal(rest.grad, first["rest"])
    with pytest.raises(ValueError, match="features_dc"):
        rast(means3D=l0["means3D"], means2D=None, opacities=l0["opacities"], scales=l0["scales"], rotations=l0["rotations"],
             shs=shs.to(dev), shs_rest=rest)
