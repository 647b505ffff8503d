"""Reference for the opt-in depth / weights gradients (GaussianRasterizationSettings.depth_weights_grad), built on the CPU
oracle without changing it.  depth = sum w_i z_i and weights = 1 - T_final = sum w_i composite like two colour channels
with colours (z_i, 1) and background 0, so each tile is blended twice with oracle.raster_oracle._blend_tile: once with the
real colours and dL/dimage, once with colours [tz, 1, 0] (tz attached to the graph), background 0 and cotangent
[dL/ddepth, dL/dweights, 0].  The per-pair dL/dG of the two calls is summed before |.| is taken for means2D_densify."""
import torch

from oracle import raster_oracle as O
from parity import GRAD_NAMES
from scenes import camera_tensors, hip_settings, make_case, oracle_settings, rel_err

TILE = O.TILE


def backward_ex(st, grad_image, grad_depth, grad_weights, inputs):
    """rasterize_backward of the oracle with the two extra cotangents ((1,H,W) each; None = zero)."""
    pre, s, dtype = st.pre, st.s, st.dtype
    W, H, gx = st.W, st.H, st.gx
    bg = s.bg.to(dtype).reshape(3)
    zero3 = torch.zeros(3, dtype=dtype)
    gimg = torch.zeros(3, H, W, dtype=dtype) if grad_image is None else grad_image.to(dtype)
    gD = torch.zeros(1, H, W, dtype=dtype) if grad_depth is None else grad_depth.to(dtype).reshape(1, H, W)
    gA = torch.zeros(1, H, W, dtype=dtype) if grad_weights is None else grad_weights.to(dtype).reshape(1, H, W)
    gext = torch.cat([gD, gA, torch.zeros(1, H, W, dtype=dtype)], 0)
    P = pre.xy.shape[0]
    tz = pre.extras["tz"]
    leaves = [t.detach().clone().requires_grad_(True) for t in (pre.xy, pre.conic, pre.opacity, pre.rgb, tz)]
    lxy, lcon, lop, lrgb, ltz = leaves
    acc = [torch.zeros_like(t) for t in leaves]
    absgrad = torch.zeros(P, 2, dtype=dtype)
    pl = st.point_list.to(torch.int64)
    zd = tz.detach()
    ext_rgb = torch.stack([ltz, torch.ones_like(ltz), torch.zeros_like(ltz)], 1)
    for t in st.tile_ids:
        ty, tx = divmod(t, gx)
        lo, hi = int(st.ranges[t, 0]), int(st.ranges[t, 1])
        if hi <= lo:
            continue
        ids = pl[lo:hi]
        y0, x0 = ty * TILE, tx * TILE
        hh, ww = min(TILE, H - y0), min(TILE, W - x0)
        r1 = O._blend_tile(ids, lxy, lcon, lop, lrgb, zd, bg, x0, y0, W, H, want_pairs=True, decide32=st.decide32)
        r2 = O._blend_tile(ids, lxy, lcon, lop, ext_rgb, zd, zero3, x0, y0, W, H, want_pairs=True, decide32=st.decide32)
        g1 = torch.zeros(TILE, TILE, 3, dtype=dtype)
        g1[:hh, :ww] = gimg[:, y0:y0 + hh, x0:x0 + ww].permute(1, 2, 0)
        g2 = torch.zeros(TILE, TILE, 3, dtype=dtype)
        g2[:hh, :ww] = gext[:, y0:y0 + hh, x0:x0 + ww].permute(1, 2, 0)
        loss = (r1["out"] * g1.reshape(256, 3)).sum() + (r2["out"] * g2.reshape(256, 3)).sum()
        grads = torch.autograd.grad(loss, leaves + [r1["G"], r2["G"]], allow_unused=True)
        for a, gr in zip(acc, grads[:5]):
            if gr is not None:
                a += gr
        dG = None
        for d in grads[5:]:
            if d is not None:
                dG = d if dG is None else dG + d
        if dG is not None:
            q = dG * r1["G"].detach()
            cxn = r1["gcon"].detach()
            dxx, dyy = r1["dx"].detach(), r1["dy"].detach()
            gx_pix = q * (-(cxn[None, :, 0] * dxx) - cxn[None, :, 1] * dyy)
            gy_pix = q * (-(cxn[None, :, 2] * dyy) - cxn[None, :, 1] * dxx)
            absgrad.index_add_(0, ids, torch.stack([(gx_pix * (0.5 * W)).abs().sum(0),
                                                     (gy_pix * (0.5 * H)).abs().sum(0)], 1))
    names = [n for n, t in inputs.items() if t is not None and t.requires_grad]
    tensors = [inputs[n] for n in names]
    outs = [pre.xy, pre.conic, pre.opacity, pre.rgb, tz]
    keep = [(o, a) for o, a in zip(outs, acc) if o.requires_grad]
    res = {}
    if tensors and keep:
        g = torch.autograd.grad([o for o, _ in keep], tensors, [a for _, a in keep], allow_unused=True)
        for n, t, gg in zip(names, tensors, g):
            res[n] = torch.zeros_like(t) if gg is None else gg
    res["means2D_densify"] = torch.cat([absgrad, torch.zeros(P, 1, dtype=dtype)], 1)
    return res


def leaves_of(inputs, s, dtype, want=True):
    """render_and_grad's leaf set-up: detached copies of the call tensors and the camera tensors (which override ``s``)."""
    leaf = {}
    for n in O.INPUT_NAMES:
        t = inputs.get(n)
        leaf[n] = None if t is None else t.detach().to(dtype).clone().requires_grad_(want)
    s2 = O.OracleSettings(**{**s.__dict__})
    for n in ("viewmatrix", "projmatrix", "intrinsic", "campos"):
        if leaf[n] is None:
            leaf[n] = getattr(s, n).detach().to(dtype).clone().requires_grad_(want)
        setattr(s2, n, leaf[n])
    if leaf["means2D"] is None:
        leaf["means2D"] = torch.zeros(leaf["means3D"].shape[0], 3, dtype=dtype, requires_grad=want)
    return leaf, s2


def forward(leaf, s2, dtype, discrete=None, tiles=None):
    return O.rasterize_forward(leaf["means3D"], leaf["means2D"], leaf["shift_factors"], leaf["shs"], leaf["colors_precomp"],
                               leaf["opacities"], leaf["scales"], leaf["rotations"], leaf["cov3D_precomp"], s2, dtype,
                               discrete, tiles)


def render_and_grad_ex(inputs, s, grad_image, grad_depth, grad_weights, dtype=torch.float32, discrete=None, tiles=None):
    leaf, s2 = leaves_of(inputs, s, dtype)
    st = forward(leaf, s2, dtype, discrete, tiles)
    return st, backward_ex(st, grad_image, grad_depth, grad_weights, leaf)


def oracle_inputs(scene, shift=None, colors=None, cov3D=None):
    inp = dict(scene)
    inp["shift_factors"] = torch.zeros(3) if shift is None else shift
    if colors is not None:
        inp["colors_precomp"] = colors; inp["shs"] = None
    if cov3D is not None:
        inp["cov3D_precomp"] = cov3D; inp["scales"] = None; inp["rotations"] = None
    return inp


def run_hip_ex(scene, cam, deg, g_img, g_depth, g_weights, bg=None, shift=None, colors=None, cov3D=None, depth_key="z",
               tile_bounds="opacity", binning="auto", frozen_camera=False, depth_weights_grad=True, scale_modifier=1.0,
               clamp_grad="stock", conic_grad="stock"):
    """Forward + backward through the product op with depth_weights_grad; any cotangent may be None (that output is not in the
    loss; all three None: the forward alone, grads is None).  Returns (outputs, grads)."""
    from bags_raster import GaussianRasterizer
    dev = torch.device("cuda")
    t = {k: v.to(dev).clone().requires_grad_(True) for k, v in scene.items()}
    ct = {k: v.clone().requires_grad_(not frozen_camera) for k, v in camera_tensors(cam, dev).items()}
    P = t["means3D"].shape[0]
    m2 = torch.zeros(P, 3, device=dev, requires_grad=True)
    m2d = None if frozen_camera else torch.zeros(P, 3, device=dev, requires_grad=True)
    sf = None if frozen_camera else (torch.zeros(3) if shift is None else shift).to(dev).requires_grad_(True)
    col = None if colors is None else colors.to(dev).clone().requires_grad_(True)
    cov = None if cov3D is None else cov3D.to(dev).clone().requires_grad_(True)
    st = hip_settings(cam, deg, dev, bg=bg, scale_modifier=scale_modifier, depth_key=depth_key, tensors=ct, tile_bounds=tile_bounds,
                      binning=binning, clamp_grad=clamp_grad, conic_grad=conic_grad)
    st = st._replace(depth_weights_grad=depth_weights_grad)
    outs = GaussianRasterizer(st)(means3D=t["means3D"], means2D=m2, means2D_densify=m2d, shift_factors=sf,
                                  shs=None if col is not None else t["shs"], colors_precomp=col, opacities=t["opacities"],
                                  scales=None if cov is not None else t["scales"], rotations=None if cov is not None else t["rotations"],
                                  cov3D_precomp=cov)
    pairs = [(o, g) for o, g in ((outs[0], g_img), (outs[2], g_depth), (outs[3], g_weights)) if g is not None]
    if not pairs:
        return [o.detach().cpu() for o in outs], None
    torch.autograd.backward([o for o, _ in pairs], [g.to(dev) for _, g in pairs])
    src = dict(means3D=t["means3D"], means2D=m2, means2D_densify=m2d, shift_factors=sf, shs=t["shs"], colors_precomp=col,
               opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"], cov3D_precomp=cov, **ct)
    grads = {k: (None if v is None or v.grad is None else v.grad.detach().cpu()) for k, v in src.items()}
    return [o.detach().cpu() for o in outs], grads


def cotangents(H, W, seed, image=True, depth=True, weights=True, mask=None):
    gen = torch.Generator().manual_seed(seed)
    gi = torch.randn(3, H, W, generator=gen) if image else None
    gd = torch.randn(1, H, W, generator=gen) * 0.3 if depth else None
    gw = torch.randn(1, H, W, generator=gen) if weights else None
    if mask is not None:
        gi, gd, gw = [None if x is None else x * mask for x in (gi, gd, gw)]
    return gi, gd, gw


ORACLE_KW = ("bg", "scale_modifier", "depth_key", "tile_bounds", "clamp_grad", "conic_grad")


def compare_ex(scene, cam, deg, seed=1, check_fp64=True, tiles=None, image=True, depth=True, weights=True, return_oracle=False, **kw):
    """HIP (depth_weights_grad) against the fp32 reference and its fp64 replay: relative error of every gradient tensor.  The forward
    is held to itself here (asserted: the five outputs with the keyword on are torch.equal to those with it off; parity.compare holds
    them to the oracle).  return_oracle: also the fp32 reference's lists and preprocessed values, for host derivations that
    must not lean on the code under test (parity.chunk_quadrant_counts)."""
    H, W = cam.image_height, cam.image_width
    mask = None
    if tiles is not None:
        gx = (W + 15) // 16
        mask = torch.zeros(H, W)
        for t in tiles.tolist():
            ty, tx = divmod(t, gx)
            mask[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = 1.0
    gi, gd, gw = cotangents(H, W, seed, image, depth, weights, mask)
    outs, grads = run_hip_ex(scene, cam, deg, gi, gd, gw, **kw)
    outs_off, _ = run_hip_ex(scene, cam, deg, None, None, None, **{**kw, "depth_weights_grad": False})
    s = oracle_settings(cam, deg, **{k: v for k, v in kw.items() if k in ORACLE_KW})
    inp = oracle_inputs(scene, kw.get("shift"), kw.get("colors"), kw.get("cov3D"))
    st32, gr32 = render_and_grad_ex(inp, s, gi, gd, gw, torch.float32, tiles=tiles)
    for name, a, b in zip(("image", "radii", "depth", "weights", "mean2D"), outs, outs_off):
        assert torch.equal(a, b), f"forward output {name} differs between depth_weights_grad on and off"
    rep = {"grad_rel_fp32": {k: rel_err(grads[k], gr32[k]) for k in GRAD_NAMES if grads.get(k) is not None and k in gr32}}
    if check_fp64:
        _, gr64 = render_and_grad_ex(inp, s, gi, gd, gw, torch.float64, discrete=O.discrete_of(st32), tiles=tiles)
        rep["grad_rel_fp64"] = {k: rel_err(grads[k], gr64[k]) for k in GRAD_NAMES if grads.get(k) is not None and k in gr64}
        rep["oracle32_vs_64"] = {k: rel_err(gr32[k], gr64[k]) for k in GRAD_NAMES if k in gr32 and k in gr64}
    if return_oracle:
        return rep, oracle_lists(st32)
    return rep


def oracle_lists(st):
    """What the host derivations need of an oracle forward: its lists, ranges, n_contrib and preprocessed xy / conic / opacity."""
    pre = st.pre
    return dict(point_list=st.point_list.numpy(), ranges=st.ranges.numpy(), n_contrib=st.n_contrib.numpy(), gx=st.gx,
                xy=pre.xy.detach().double().numpy(), conic=pre.conic.detach().double().numpy(),
                opacity=pre.opacity.detach().double().numpy())


def oracle_forward(scene, cam, deg, **kw):
    """The fp32 oracle's forward alone (no gradients) with compare_ex's keywords."""
    s = oracle_settings(cam, deg, **{k: v for k, v in kw.items() if k in ORACLE_KW})
    leaf, s2 = leaves_of(oracle_inputs(scene, kw.get("shift"), kw.get("colors"), kw.get("cov3D")), s, torch.float32, want=False)
    with torch.no_grad():
        return forward(leaf, s2, torch.float32)


def bwd_constants():
    """The sizes launch_blend_bwd and blend_bwd_scan_kernel decide with, read from csrc/blend.hip (the shipped build defines none of
    them on the command line)."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "bundle-adjusting-gaussian-splatting_amd", "csrc", "blend.hip")).read()
    return {n: int(re.search(r"#define\s+%s\s+(\d+)" % n, src).group(1)) for n in
            ("BCHUNK", "BSLOTS", "WCHUNK", "WSLOTS", "BWD_SPARSE_PER_TILE", "BWD_DENSE_PER_TILE", "COMPACT_DENSITY_NUM", "EXTRA_SLOTS")}


def bwd_path(n_instances, T, tile_bounds, extra=True, binning="auto"):
    """launch_blend_bwd's choice for a backward of n_instances list entries on T tiles, as the code makes it: the chunk geometry
    (sparse: WCHUNK / WSLOTS up to BWD_SPARSE_PER_TILE instances per tile; the stock tile rule on the tile-binned path stages only
    its record holders and scales the count by COMPACT_DENSITY_NUM / 5), the dense-scene mode, and the resulting chunk length CH and
    slots SL per wave copy (8 fewer for the compacted lists, EXTRA_SLOTS fewer with the depth / weights cotangents)."""
    c = bwd_constants()
    compact = binning != "radix" and tile_bounds != "opacity"
    x5 = n_instances * (c["COMPACT_DENSITY_NUM"] if compact else 5)
    sparse = x5 <= 5 * c["BWD_SPARSE_PER_TILE"] * T
    SL = (c["WSLOTS"] if sparse else c["BSLOTS"]) - (8 if compact else 0) - (c["EXTRA_SLOTS"] if extra else 0)
    return dict(compact=compact, sparse=sparse, dense=n_instances > c["BWD_DENSE_PER_TILE"] * T,
                CH=c["WCHUNK"] if sparse else c["BCHUNK"], SL=SL, SL_default=SL + (c["EXTRA_SLOTS"] if extra else 0))


def scene_chunks(scene, cam, deg, tile_bounds="opacity", **kw):
    """(bwd_path of the scene, its chunks as parity.chunk_quadrant_counts lists them, the oracle forward), from the oracle alone."""
    from parity import chunk_quadrant_counts
    st = oracle_forward(scene, cam, deg, tile_bounds=tile_bounds, **kw)
    o = oracle_lists(st)
    path = bwd_path(int(st.point_list.numel()), st.gx * st.gy, tile_bounds)
    rec = None
    if path["compact"]:          # the record holders: the (tile, Gaussian) pairs of the opacity rule's lists
        ro = oracle_lists(oracle_forward(scene, cam, deg, tile_bounds="opacity", **kw))
        rec = (ro["point_list"], ro["ranges"])
    chunks = chunk_quadrant_counts(o["point_list"], o["ranges"], o["n_contrib"], o["xy"], o["conic"], o["opacity"], o["gx"], path["CH"], rec)
    return path, chunks, st


# ---- small scenes, each built to take one path of the EXTRA backward (tests/test_depth_grad_cpu.py proves the path from the oracle
# alone, tests/test_depth_grad_gpu.py holds the kernels to the oracle on it).  All on a 64 x 48 image (12 tiles) unless named otherwise.
def _faint(scene):
    scene["opacities"] = scene["opacities"] * 0.2
    return scene


def _huge_and_small(n_huge, n_small, sm_small, seed=21):
    """n_huge faint screen-filling splats (every one reaches every quadrant of every tile) among n_small small ones (each reaches a
    quadrant or two): the small ones fill a chunk's staged slots without filling any one wave copy."""
    a, cam = make_case(n_huge, 64, 48, 8.0, 1, seed=seed)
    b, _ = make_case(n_small, 64, 48, sm_small, 1, seed=seed + 1)
    return _faint({k: torch.cat([a[k], b[k]], 0) for k in a}), cam


BAND_DENSE = {"opacity": (160, 1500, 1.0), "aabb": (150, 1000, 2.0)}


def path_scene(name, tile_bounds="opacity"):
    """(scene, camera, SH degree) of a named path scene."""
    if name == "band_sparse":          # chunks of 240, some with SL - 16 < reach <= SL: one pass in the default kernel, two with the extras
        return _huge_and_small(115, 1500, 0.5) + (1,)
    if name == "band_dense":           # the same band in the 224-splat geometry (one scene per tile rule: the stock rule needs 500 per tile)
        return _huge_and_small(*BAND_DENSE[tile_bounds]) + (1,)
    if name == "overflow":             # test_wide_chunks_that_overflow_a_wave_copy's scene: every full chunk in two halves
        scene, cam = make_case(420, 64, 48, 8.0, 1, seed=21)
        return _faint(scene), cam, 1
    if name == "dense_mode":           # the same family above BWD_DENSE_PER_TILE: live bytes instead of zero records
        scene, cam = make_case(600, 64, 48, 8.0, 1, seed=21)
        return _faint(scene), cam, 1
    if name == "saturated":            # test_saturated_alpha_and_early_termination's scene
        scene, cam = make_case(800, 96, 96, 6.0, 1, seed=11)
        scene["opacities"] = torch.full_like(scene["opacities"], 0.999)
        return scene, cam, 1
    raise KeyError(name)
