"""No-GPU checks of the opt-in depth / weights gradients (ABI 11): the reference in tests/depth_oracle.py against fp64
central differences and the closed form of d(weights)/d(alpha), and the C / Python surface of the feature."""
import ctypes as C
import os

import pytest
import torch

from bags_raster import _lib
from oracle import raster_oracle as O
from depth_oracle import backward_ex, bwd_constants, bwd_path, forward, leaves_of, oracle_forward, path_scene, scene_chunks
from scenes import make_case, oracle_settings


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def test_abi_11_exports_bags_backward_ex(lib):
    assert _lib.ABI_VERSION == 11 and lib.bags_abi_version() == 11
    assert hasattr(lib, "bags_backward_ex") and "bags_backward_ex" in _lib.SYMBOLS
    assert C.sizeof(_lib.BagsExtraGrads) == 16
    # the two structs the ABI tests pin do not grow
    assert C.sizeof(_lib.BagsSettings) == 14 * 4 + 5 * 8
    assert C.sizeof(_lib.BagsBackwardArgs) == 4 * 8 + 14 * 8 + 8 + 8 + 8 + 8 + 8


def _call_args():
    buf = (C.c_char * 4096)()
    addr = C.addressof(buf)
    s = _lib.BagsSettings(16, 16, 0.5, 0.5, 1.0, 0, 1, 0, 0, 0, 1, 0, 0, 0, addr, addr, addr, addr, addr)
    i = _lib.BagsInputs(0, None, None, None, None, None, None, None, None, None, None)
    st = _lib.BagsState(addr, 1 << 40, addr, 1 << 40, addr, 1 << 40)
    a = _lib.BagsBackwardArgs()
    a.workspace, a.workspace_bytes = addr, 1 << 40
    return buf, addr, s, i, st, a


def test_backward_ex_argument_errors(lib):
    """Reported before anything is enqueued (no GPU touched): validation never dereferences the host pointers given here."""
    buf, addr, s, i, st, a = _call_args()
    # no cotangent at all: neither grad_color nor an extra one
    x = _lib.BagsExtraGrads(None, None)
    assert lib.bags_backward_ex(C.byref(s), C.byref(i), C.byref(st), C.byref(a), C.byref(x), None) == -1
    assert b"grad_color must be given" in lib.bags_last_error() and b"grad_depth" in lib.bags_last_error()
    assert lib.bags_backward_ex(C.byref(s), C.byref(i), C.byref(st), C.byref(a), None, None) == -1
    assert b"grad_color must be given" in lib.bags_last_error()
    # with a depth cotangent and no grad_color the call gets past that check: the next defect (phase) is the one reported
    x.grad_depth = addr
    a.phase = 3
    assert lib.bags_backward_ex(C.byref(s), C.byref(i), C.byref(st), C.byref(a), C.byref(x), None) == -1
    assert b"phase" in lib.bags_last_error(), lib.bags_last_error()
    # ... and the same for weights alone
    x.grad_depth, x.grad_weights = None, addr
    assert lib.bags_backward_ex(C.byref(s), C.byref(i), C.byref(st), C.byref(a), C.byref(x), None) == -1
    assert b"phase" in lib.bags_last_error(), lib.bags_last_error()
    # bags_backward itself still requires grad_color
    assert lib.bags_backward(C.byref(s), C.byref(i), C.byref(st), C.byref(a), None) == -1
    assert b"grad_color must be given" in lib.bags_last_error()
    del buf


def test_depth_weights_grad_keyword():
    import inspect
    from bags_raster import GaussianRasterizationSettings, GaussianRasterizer
    from bags_raster.render import render
    f = GaussianRasterizationSettings._fields
    assert f[-1] == "depth_weights_grad" and GaussianRasterizationSettings._field_defaults["depth_weights_grad"] is False
    assert inspect.signature(render).parameters["depth_weights_grad"].default is False
    # every tensor on the machine's device: with a GPU the keyword is then the call's only defect (a CPU bg next to CUDA tensors was
    # reported first: "bg is on cpu"), without one the device check comes first
    x = torch.zeros(4, 3, device="cuda" if torch.cuda.is_available() else "cpu")
    dev = x.device
    eye = torch.eye(4, device=dev)
    st = GaussianRasterizationSettings(32, 32, 0.5, 0.5, torch.zeros(3, device=dev), 1.0, eye, eye, eye, 0, torch.zeros(3, device=dev),
                                       False, False, 0, depth_weights_grad="yes")
    from bags_raster.rasterizer import _Packed
    with pytest.raises((ValueError, RuntimeError), match="depth_weights_grad must be True or False" if x.is_cuda else "AMD GPU"):
        _Packed(st, x, None, None, None, x, torch.ones_like(x[:, :1]), x, torch.zeros(4, 4, device=dev), None, eye, eye, eye,
                torch.zeros(3, device=dev))
    assert GaussianRasterizer is not None


def _tiny_case():
    scene, cam = make_case(24, 32, 32, 3.0, 1, seed=5, dist=3.0)
    scene["opacities"] = scene["opacities"] * 0.8
    return scene, cam


def _loss_fp64(scene, cam, gi, gd, gw, shift, discrete):
    """L = <gi, image> + <gd, depth> + <gw, weights> of the fp64 oracle forward, with the fp32 run's lists replayed."""
    s = oracle_settings(cam, 1, clamp_grad="exact", conic_grad="exact")
    inp = dict(scene); inp["shift_factors"] = shift
    leaf, s2 = leaves_of(inp, s, torch.float64, want=False)
    st = forward(leaf, s2, torch.float64, discrete)
    return ((st.image * gi).sum() + (st.depth_img * gd).sum() + (st.weights * gw).sum()).item()


def test_reference_matches_central_differences():
    """The two-call reference against fp64 central differences of <g, image> + <gD, depth> + <gA, weights> on a tiny scene, for
    means3D, opacities, the viewmatrix and the shift factors (the depth term is what reaches dL/dz).  Pairs within the step of a
    threshold (alpha = 1/255, T = 1e-4) would make a difference quotient meaningless: the scene is checked to have none."""
    torch.manual_seed(0)
    scene, cam = _tiny_case()
    H, W = cam.image_height, cam.image_width
    gen = torch.Generator().manual_seed(9)
    gi = torch.randn(3, H, W, generator=gen, dtype=torch.float64)
    gd = torch.randn(1, H, W, generator=gen, dtype=torch.float64)
    gw = torch.randn(1, H, W, generator=gen, dtype=torch.float64)
    shift = torch.tensor([0.01, -0.004, 0.002])
    # (the exact derivatives of the frustum clamp and the conic inverse: the stock rules are what upstream differentiates, not
    # the derivative a difference quotient measures)
    s = oracle_settings(cam, 1, clamp_grad="exact", conic_grad="exact")
    inp = dict(scene); inp["shift_factors"] = shift
    leaf32, s32 = leaves_of(inp, s, torch.float32, want=False)
    discrete = O.discrete_of(forward(leaf32, s32, torch.float32))
    leaf, s2 = leaves_of(inp, s, torch.float64)
    st = forward(leaf, s2, torch.float64, discrete)
    # no pair near a threshold: every alpha at least 1e-3 away from 1/255 (relative), T never near 1e-4
    assert float(st.final_T.min()) > 1e-3
    g = backward_ex(st, gi, gd, gw, leaf)
    h = 1e-6
    checked = 0
    for name, idxs in (("means3D", [(i, c) for i in range(0, 24, 3) for c in range(3)]), ("opacities", [(i, 0) for i in range(0, 24, 2)]),
                       ("viewmatrix", [(3, 0), (3, 1), (3, 2), (0, 2), (2, 2)]), ("shift_factors", [(0,), (1,)])):
        for ix in idxs:
            fp, fm = dict(inp), dict(inp)
            for f, sgn in ((fp, 1.0), (fm, -1.0)):
                if name == "viewmatrix":
                    v = s.viewmatrix.detach().double().clone(); v[ix] += sgn * h
                    f["viewmatrix"] = v
                else:
                    t = inp[name].detach().double().clone(); t[ix] += sgn * h
                    f[name] = t
            lp = _loss_fp64(fp, cam, gi, gd, gw, fp["shift_factors"], discrete)
            lm = _loss_fp64(fm, cam, gi, gd, gw, fm["shift_factors"], discrete)
            fd = (lp - lm) / (2 * h)
            an = float(g[name][ix])
            assert abs(fd - an) <= 1e-5 * max(1.0, abs(an)) + 2e-6 * max(1.0, abs(fd)), (name, ix, fd, an)
            checked += 1
    assert checked > 40
    # the depth term is not silently zero: without it the depth-only derivative differs
    leaf, s2 = leaves_of(inp, s, torch.float64)
    g0 = backward_ex(forward(leaf, s2, torch.float64, discrete), None, gd, None, leaf)
    assert float(g0["means3D"].abs().sum()) > 0 and float(g0["viewmatrix"].abs().sum()) > 0


def test_weights_cotangent_has_the_closed_form():
    """d(1 - T_final)/d alpha_i = T_final / (1 - alpha_i) on every contributing (pixel, splat) pair: the reference's second
    blend (colours [z, 1, 0], cotangent [0, gA, 0]) must give dL/dG = gA o T_final / (1 - alpha)."""
    scene, cam = _tiny_case()
    s = oracle_settings(cam, 1)
    inp = dict(scene); inp["shift_factors"] = torch.zeros(3)
    leaf, s2 = leaves_of(inp, s, torch.float64, want=False)
    st = forward(leaf, s2, torch.float64)
    pre = st.pre
    ext = torch.stack([pre.extras["tz"], torch.ones_like(pre.extras["tz"]), torch.zeros_like(pre.extras["tz"])], 1).detach()
    gA = torch.randn(256, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    n_pairs = 0
    for t in range(st.gx * st.gy):
        lo, hi = int(st.ranges[t, 0]), int(st.ranges[t, 1])
        if hi <= lo:
            continue
        ty, tx = divmod(t, st.gx)
        ids = st.point_list[lo:hi].to(torch.int64)
        xy = pre.xy.detach().clone().requires_grad_(True)      # (so that G is a node of the graph)
        r = O._blend_tile(ids, xy, pre.conic.detach(), pre.opacity.detach(), ext, pre.extras["tz"].detach(),
                          torch.zeros(3, dtype=torch.float64), tx * 16, ty * 16, st.W, st.H, want_pairs=True)
        G = r["G"]
        (dG,) = torch.autograd.grad((r["out"][:, 1] * gA).sum(), [G])
        op = pre.opacity.detach()[ids].reshape(-1)
        alpha = torch.clamp(op[None, :] * G.detach(), max=0.99)
        Tf = r["T_final"].detach()
        want = gA[:, None] * op[None, :] * Tf[:, None] / (1.0 - alpha)
        c = r["contrib"]
        assert torch.allclose(dG[c], want[c], rtol=1e-9, atol=1e-12)
        assert bool((dG[~c] == 0).all())
        n_pairs += int(c.sum())
    assert n_pairs > 100


# ---- the path scenes of tests/test_depth_grad_gpu.py: that each takes the path it is named for, from the oracle alone
def _quadrant_counts(name, tile_bounds):
    scene, cam, deg = path_scene(name, tile_bounds)
    path, chunks, st = scene_chunks(scene, cam, deg, tile_bounds=tile_bounds)
    return path, [c for per_tile in chunks.values() for c in per_tile], st, cam


def test_launch_constants_are_the_ones_the_scenes_were_tuned_for():
    """bwd_path reads them from csrc/blend.hip; the counts in the docstrings below were found with these."""
    assert bwd_constants() == dict(BCHUNK=224, BSLOTS=176, WCHUNK=240, WSLOTS=168, BWD_SPARSE_PER_TILE=300, BWD_DENSE_PER_TILE=480,
                                   COMPACT_DENSITY_NUM=3, EXTRA_SLOTS=16)
    # launch_blend_bwd's comparison, both tile rules: 5 n <= 1500 T, and 3 n <= 1500 T for the compacted lists
    assert bwd_path(3600, 12, "opacity")["sparse"] and not bwd_path(3601, 12, "opacity")["sparse"]
    assert bwd_path(6000, 12, "aabb")["sparse"] and not bwd_path(6001, 12, "aabb")["sparse"]
    assert not bwd_path(5760, 12, "opacity")["dense"] and bwd_path(5761, 12, "aabb")["dense"]
    assert [bwd_path(n, 12, tb)["SL"] for n, tb in ((1, "opacity"), (1, "aabb"), (9999, "opacity"), (9999, "aabb"))] == [152, 144, 160, 152]
    assert bwd_path(1, 12, "aabb", binning="radix")["SL"] == 152           # the radix path's lists are not compacted


@pytest.mark.parametrize("name,tile_bounds,sparse,dense", [("band_sparse", "opacity", True, False), ("band_sparse", "aabb", True, False),
                                                            ("band_dense", "opacity", False, False), ("band_dense", "aabb", False, True)])
def test_band_scenes_have_chunks_only_the_extras_split(name, tile_bounds, sparse, dense):
    """A chunk whose fullest quadrant is reached by more than SL - 16 and at most SL staged splats runs in one pass in the default
    kernel and in two halves with the extras (SL: the default instance's slots per wave copy).  At least 3 such chunks per scene, and
    at least 3 of them two or more away from either end of the band (the host evaluates the reach rule in fp64, the forward in fp32).
    Found (instances per tile; geometry; chunks: one pass / in the band / over SL also by default; the band's counts):
      band_sparse opacity  273.0   240 / 168   9 /  7 /  2   155 155 155 159 161 166 166   of (152, 168]
      band_sparse aabb     388.9   240 / 160   8 /  5 /  5   151 155 155 155 159           of (144, 160]
      band_dense  opacity  376.4   224 / 176  19 /  4 /  6   168 169 171 172               of (160, 176]
      band_dense  aabb     738.6   224 / 168  11 /  5 / 14   155 155 156 156 164           of (152, 168]
    (the stock rule counts 3/5 of its list as record holders: sparse up to 500 per tile, so its dense-geometry scene is also past 480)"""
    path, chunks, st, _ = _quadrant_counts(name, tile_bounds)
    per_tile = st.point_list.numel() / (st.gx * st.gy)
    assert path["sparse"] == sparse and path["dense"] == dense and path["compact"] == (tile_bounds == "aabb"), (per_tile, path)
    assert (per_tile <= (500 if tile_bounds == "aabb" else 300)) == sparse and (per_tile > 480) == dense, per_tile
    SL = path["SL_default"]
    band = sorted(q for _, q in chunks if SL - 16 < q <= SL)
    print(name, tile_bounds, per_tile, path, len(chunks), band)
    assert len(band) >= 3 and sum(SL - 16 + 3 <= q <= SL - 2 for q in band) >= 3, band
    assert any(q <= SL - 16 for _, q in chunks) and any(q > SL for _, q in chunks)      # and both neighbours of the band


def test_the_1500_splat_family_has_band_chunks_too():
    """make_case(1500, 128, 96, 1.0, 3), the one family of the older oracle comparisons of tests/test_depth_grad_gpu.py: sparse geometry
    only (154 .. 156 instances per tile), yet 6 to 9 of its ~60 chunks lie in (152, 168] -- seed 11 (the sh3 case): 153 154 154 154 156
    157 161 165 168; seed 14 (test_zero_extra_cotangents_leave_the_image_gradients, which cites the two-half branch): 153 155 155 157
    159 159 163.  So that family does run the branch, in the 240 / 168 geometry alone; the scenes above add the 224 / 176 geometry, chunks
    that split in every instance and the dense-scene mode."""
    for seed, n_band in ((11, 9), (14, 7)):
        scene, cam = make_case(1500, 128, 96, 1.0, 3, seed=seed)
        path, chunks, st = scene_chunks(scene, cam, 3)
        assert path["sparse"] and not path["dense"] and path["SL_default"] == 168
        band = [q for per_tile in chunks.values() for _, q in per_tile if 152 < q <= 168]
        assert abs(len(band) - n_band) <= 2 and len(band) >= 3, band        # (+-2: counts at an end of the band, fp64 here / fp32 there)


@pytest.mark.parametrize("tile_bounds", ["opacity", "aabb"])
def test_overflow_scene_splits_every_full_chunk(tile_bounds):
    """Every chunk that stages a full CH splats is over SL (with and without the extras): 12 of 12 with either rule, at 377.5 (224 / 160,
    opacity rule) and 420.0 (240 / 144: sparse for the stock rule) instances per tile; the 12 second chunks are shorter and 6 of them
    land in the band."""
    path, chunks, st, _ = _quadrant_counts("overflow", tile_bounds)
    assert path["sparse"] == (tile_bounds == "aabb") and not path["dense"]
    full = [q for n, q in chunks if n == path["CH"]]
    assert len(full) >= 12 and all(q > path["SL_default"] for q in full), full


def test_dense_mode_scene_is_past_the_threshold():
    """525.5 instances per tile (> 480): live bytes, no zero records; 24 full chunks, all split."""
    path, chunks, st, _ = _quadrant_counts("dense_mode", "opacity")
    assert path["dense"] and not path["sparse"] and st.point_list.numel() > 480 * st.gx * st.gy
    assert sum(n == 224 and q > 176 for n, q in chunks) >= 12


def test_saturated_scene_stops_early():
    """Opaque splats: the oracle's n_contrib is below the tile's list length on every pixel (1.000 of them; the bar is half)."""
    scene, cam, deg = path_scene("saturated")
    st = oracle_forward(scene, cam, deg)
    lens = (st.ranges[:, 1] - st.ranges[:, 0]).view(st.gy, st.gx)
    per_pixel = lens[torch.arange(cam.image_height)[:, None] // 16, torch.arange(cam.image_width)[None, :] // 16]
    assert float((st.n_contrib < per_pixel).float().mean()) > 0.5
    assert float(st.final_T.median()) < 1e-3                          # most pixels ran down to the T < 1e-4 stop ...
    assert int((st.n_contrib > 0).sum()) == st.n_contrib.numel()      # ... and every pixel has a contributor


@pytest.mark.parametrize("W,H", [(100, 70), (17, 33)])
def test_ragged_scenes_overhang(W, H):
    """The right column and the bottom row of tiles overhang the image and hold contributors (100 x 70: 7 x 5 tiles, 17 x 33: 2 x 3)."""
    scene, cam = make_case(800, W, H, 2.0, 2, seed=W)
    st = oracle_forward(scene, cam, 2)
    assert W % 16 and H % 16 and (st.gx, st.gy) == ((W + 15) // 16, (H + 15) // 16)
    assert int((st.n_contrib[:, (st.gx - 1) * 16:] > 0).sum()) > 0 and int((st.n_contrib[(st.gy - 1) * 16:, :] > 0).sum()) > 0


def test_clamp_scene_has_clamped_gaussians_in_its_lists():
    """settings[clamp_exact]: 1.3 x the field of view is crossed by Gaussians that reach the image (the two clamp semantics differ
    only there)."""
    import math
    from scenes import camera_tensors
    scene, cam = make_case(1500, 96, 64, 2.0, 1, seed=3, dist=2.5)
    st = oracle_forward(scene, cam, 1, clamp_grad="exact")
    t = torch.cat([scene["means3D"], torch.ones(1500, 1)], 1) @ camera_tensors(cam)["viewmatrix"]
    clamped = ((t[:, 0] / t[:, 2]).abs() > 1.3 * math.tan(cam.FoVx / 2)) | ((t[:, 1] / t[:, 2]).abs() > 1.3 * math.tan(cam.FoVy / 2))
    listed = torch.zeros(1500, dtype=torch.bool)
    listed[st.point_list.long()] = True
    print(int((clamped & listed).sum()))
    assert int((clamped & listed).sum()) > 50
