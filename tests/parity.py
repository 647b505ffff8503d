"""HIP-vs-oracle comparison used by the -m gpu tests and __graft_entry__.smoke()."""
import torch

from oracle import raster_oracle as O
from scenes import camera_tensors, hip_settings, oracle_settings, rel_err

import json
import os


def dump_report(name, rep):
    """Append a parity report to gpurun_out/parity_reports.jsonl when that directory exists (GPU box / local runs), so the
    measured errors of a green run can be quoted in DESIGN.md and profiles/."""
    d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(d):
        try:
            with open(os.path.join(d, "parity_reports.jsonl"), "a") as f:
                f.write(json.dumps({"test": name, **{k: v for k, v in rep.items() if not torch.is_tensor(v)}}, default=str) + "\n")
        except OSError:
            pass


GRAD_NAMES = ("means3D", "means2D", "means2D_densify", "shift_factors", "shs", "colors_precomp", "opacities", "scales",
              "rotations", "cov3D_precomp", "viewmatrix", "projmatrix", "intrinsic", "campos")


def run_hip(scene, cam, deg, grad_image=None, device="cuda", bg=None, shift=None, colors=None, cov3D=None,
            scale_modifier=1.0, depth_key="z", debug=False, means2D=None, tile_bounds="opacity", binning="auto",
            clamp_grad="stock", frozen_camera=False, conic_grad="stock"):
    """Forward (+ backward) through the product op.  Returns (outputs, grads dict, views dict).
    frozen_camera: the op as the reference calls it when neither --opt_cam nor --opt_intrinsic is given (train.py:472-485 steps the
    camera leaves only under those flags; BASELINE config 2, "fixed pose"): the four camera tensors do not require a gradient,
    means2D_densify and shift_factors are None -- the library then gets NULL for grad_viewmatrix .. grad_campos,
    grad_means2D_densify (the backward's instantiation without the abs sums) and grad_shift_factors."""
    from bags_raster import GaussianRasterizer, debug_views
    dev = torch.device(device)
    want = grad_image is not None
    t = {k: v.to(dev).clone().requires_grad_(want) for k, v in scene.items()}
    ct = {k: v.clone().requires_grad_(want and not frozen_camera) for k, v in camera_tensors(cam, dev).items()}
    P = t["means3D"].shape[0]
    m2 = (torch.zeros(P, 3) if means2D is None else means2D).to(dev).requires_grad_(want)
    m2d = None if frozen_camera else torch.zeros(P, 3, device=dev, requires_grad=want)
    sf = None if frozen_camera else (torch.zeros(3) if shift is None else shift).to(dev).requires_grad_(want)
    col = None if colors is None else colors.to(dev).clone().requires_grad_(want)
    cov = None if cov3D is None else cov3D.to(dev).clone().requires_grad_(want)
    st = hip_settings(cam, deg, dev, bg=bg, scale_modifier=scale_modifier, depth_key=depth_key, tensors=ct, debug=debug,
                      tile_bounds=tile_bounds, binning=binning, clamp_grad=clamp_grad, conic_grad=conic_grad)
    rast = GaussianRasterizer(st)
    kw = dict(means3D=t["means3D"], means2D=m2, means2D_densify=m2d, shift_factors=sf,
              shs=None if col is not None else t["shs"], colors_precomp=col, opacities=t["opacities"],
              scales=None if cov is not None else t["scales"], rotations=None if cov is not None else t["rotations"],
              cov3D_precomp=cov)
    outs = rast(**kw)
    grads = None
    if want:
        outs[0].backward(grad_image.to(dev))
        src = dict(means3D=t["means3D"], means2D=m2, means2D_densify=m2d, shift_factors=sf, shs=t["shs"],
                   colors_precomp=col, opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"],
                   cov3D_precomp=cov, **ct)
        grads = {k: (None if v is None or v.grad is None else v.grad.detach().cpu()) for k, v in src.items()}
    with torch.no_grad():
        views = debug_views(st, *[None if kw[k] is None else kw[k].detach() for k in
                                  ("means3D", "means2D", "shift_factors", "shs", "colors_precomp", "opacities",
                                   "scales", "rotations", "cov3D_precomp")])
    views = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in views.items() if k != "outputs"}
    return [o.detach().cpu() for o in outs], grads, views


def run_oracle(scene, cam, deg, grad_image=None, dtype=torch.float32, bg=None, shift=None, colors=None, cov3D=None,
               scale_modifier=1.0, depth_key="z", discrete=None, means2D=None, tile_bounds="opacity", clamp_grad="stock",
               binning=None, frozen_camera=None, conic_grad="stock"):
    s = oracle_settings(cam, deg, bg=bg, scale_modifier=scale_modifier, depth_key=depth_key, tile_bounds=tile_bounds,
                        clamp_grad=clamp_grad, conic_grad=conic_grad)
    inp = dict(scene)
    inp["shift_factors"] = torch.zeros(3) if shift is None else shift
    if means2D is not None:
        inp["means2D"] = means2D
    if colors is not None:
        inp["colors_precomp"] = colors; inp["shs"] = None
    if cov3D is not None:
        inp["cov3D_precomp"] = cov3D; inp["scales"] = None; inp["rotations"] = None
    return O.render_and_grad(inp, s, grad_image, dtype=dtype, discrete=discrete)


def compare(scene, cam, deg, seed=1, check_fp64=True, **kw):
    """Full parity report of one case.  Integer artefacts are compared bit for bit, floats by tolerance."""
    H, W = cam.image_height, cam.image_width
    g = torch.randn(3, H, W, generator=torch.Generator().manual_seed(seed))
    outs, grads, views = run_hip(scene, cam, deg, g, **kw)
    st32, gr32 = run_oracle(scene, cam, deg, g, torch.float32, **kw)
    rep = {}
    # ---- integers: bit-exact
    rep["radii_equal"] = bool(torch.equal(outs[1], st32.radii))
    rep["tiles_touched_equal"] = bool(torch.equal(views["tiles_touched"], st32.pre.tiles_touched))
    rep["rect_equal"] = bool(torch.equal(views["rect"], st32.pre.rect))
    vis = st32.pre.visible
    d32 = st32.pre.depth.detach().float().contiguous().view(torch.int32)
    rep["depth_bits_equal"] = bool(torch.equal(views["depth_bits"][vis], d32[vis]))
    rep["num_rendered"] = (views["num_rendered"], int(st32.point_list.numel()))
    same_I = views["num_rendered"] == st32.point_list.numel()
    rep["point_list_equal"] = same_I and bool(torch.equal(views["point_list"], st32.point_list))
    rep["keys_equal"] = same_I and bool(torch.equal(views["keys_sorted"], st32.keys_sorted))
    cnt_h = views["ranges"][:, 1] - views["ranges"][:, 0]
    cnt_o = st32.ranges[:, 1] - st32.ranges[:, 0]
    nz = cnt_o > 0
    rep["ranges_equal"] = bool(torch.equal(cnt_h, cnt_o)) and bool(torch.equal(views["ranges"][nz], st32.ranges[nz]))
    nc_mis = (views["n_contrib"] != st32.n_contrib).float().mean().item()
    rep["n_contrib_mismatch_frac"] = nc_mis
    # ---- floats
    img_err = (outs[0] - st32.image).abs() / (1.0 + st32.image.abs())
    rep["image_max_err_fp32"] = img_err.max().item()
    d_err = (outs[2] - st32.depth_img).abs() / (1.0 + st32.depth_img.abs())
    w_err = (outs[3] - st32.weights).abs()
    rep["depth_max_err"], rep["weights_max_err"] = d_err.max().item(), w_err.max().item()
    rep["depth_bad_frac"] = (d_err > 1e-4).float().mean().item()       # same flipped-pair caveat as the image
    rep["weights_bad_frac"] = (w_err > 1e-4).float().mean().item()
    rep["mean2D_max_err"] = (outs[4] - st32.mean2D).abs().max().item()
    rep["grad_rel_fp32"] = {k: rel_err(grads[k], gr32[k]) for k in GRAD_NAMES if grads.get(k) is not None and k in gr32}
    if check_fp64:
        st64, gr64 = run_oracle(scene, cam, deg, g, torch.float64, discrete=O.discrete_of(st32), **kw)
        rep["grad_rel_fp64"] = {k: rel_err(grads[k], gr64[k]) for k in GRAD_NAMES if grads.get(k) is not None and k in gr64}
        rep["oracle32_vs_64"] = {k: rel_err(gr32[k], gr64[k]) for k in GRAD_NAMES if k in gr32 and k in gr64}
        img64 = st64.image.float()
        err64 = (outs[0] - img64).abs() / (1.0 + img64.abs())
        rep["image_max_err_fp64"] = err64.max().item()
        rep["oracle32_vs_64_image_max"] = ((st32.image - img64).abs() / (1.0 + img64.abs())).max().item()
        # pixels further from fp64 than 3x the fp32 oracle's worst pixel: flipped threshold pairs (alpha >= 1/255, T < 1e-4)
        rep["image_outlier_frac_fp64"] = (err64 > 3.0 * rep["oracle32_vs_64_image_max"] + 1e-5).float().mean().item()
        img_err = torch.minimum(img_err, err64)
    # A pixel counts as wrong only if it disagrees with BOTH oracles: alpha>=1/255, power<=0 and T<1e-4 are hard
    # thresholds, so an ulp of difference in exp() flips a (pixel, splat) pair in any one implementation.
    rep["image_max_err"] = img_err.max().item()
    rep["image_bad_frac"] = (img_err > 1e-5).float().mean().item()
    # the same as COUNTS of pixels, which is what assert_report holds to zero (or to a documented number of threshold pixels)
    rep["image_bad_pixels"] = int((img_err > 1e-5).any(0).sum())
    rep["depth_bad_pixels"], rep["weights_bad_pixels"] = int((d_err > 1e-4).sum()), int((w_err > 1e-4).sum())
    return rep


def sample_tiles(W, H, n, seed=0):
    """n distinct tile ids: the four corners, the centre, and a seeded random draw of the rest."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    T = gx * gy
    fixed = [0, gx - 1, (gy - 1) * gx, T - 1, (gy // 2) * gx + gx // 2]
    perm = torch.randperm(T, generator=torch.Generator().manual_seed(seed)).tolist()
    out = list(dict.fromkeys(fixed + perm))[:min(n, T)]
    return torch.tensor(sorted(out), dtype=torch.int64)


def compare_sampled(scene, cam, deg, tiles, seed=1, check_fp64=False, return_grads=False, **kw):
    """compare() for sizes at which the CPU oracle cannot blend every tile in seconds (BASELINE configs 4 and 5).

    Preprocess, binning and the sort are compared for ALL Gaussians / instances (bit-exact, as in compare()).  Blending
    is checked on the sampled tiles: the cotangent dL/dimage is zero outside them, so the HIP backward over the WHOLE
    image computes exactly what the oracle's backward over the sampled tiles computes (a zero cotangent contributes
    exact zeros), and every gradient tensor stays comparable in full."""
    H, W = cam.image_height, cam.image_width
    gx = (W + 15) // 16
    mask = torch.zeros(H, W, dtype=torch.bool)
    for t in tiles.tolist():
        ty, tx = divmod(t, gx)
        mask[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = True
    g = torch.randn(3, H, W, generator=torch.Generator().manual_seed(seed)) * mask
    outs, grads, views = run_hip(scene, cam, deg, g, **kw)
    s = oracle_settings(cam, deg, **{k: v for k, v in kw.items() if k in ("bg", "scale_modifier", "depth_key", "tile_bounds", "clamp_grad", "conic_grad")})
    inp = dict(scene)
    inp["shift_factors"] = kw.get("shift") if kw.get("shift") is not None else torch.zeros(3)
    st32, gr32 = O.render_and_grad(inp, s, g, dtype=torch.float32, tiles=tiles)
    rep = {"sampled_tiles": int(tiles.numel()), "sampled_pixels": int(mask.sum())}
    rep["radii_equal"] = bool(torch.equal(outs[1], st32.radii))
    rep["tiles_touched_equal"] = bool(torch.equal(views["tiles_touched"], st32.pre.tiles_touched))
    rep["rect_equal"] = bool(torch.equal(views["rect"], st32.pre.rect))
    vis = st32.pre.visible
    d32 = st32.pre.depth.detach().float().contiguous().view(torch.int32)
    rep["depth_bits_equal"] = bool(torch.equal(views["depth_bits"][vis], d32[vis]))
    rep["num_rendered"] = (views["num_rendered"], int(st32.point_list.numel()))
    same_I = views["num_rendered"] == st32.point_list.numel()
    rep["point_list_equal"] = same_I and bool(torch.equal(views["point_list"], st32.point_list))
    rep["keys_equal"] = same_I and bool(torch.equal(views["keys_sorted"], st32.keys_sorted))
    cnt_h = views["ranges"][:, 1] - views["ranges"][:, 0]
    cnt_o = st32.ranges[:, 1] - st32.ranges[:, 0]
    nz = cnt_o > 0
    rep["ranges_equal"] = bool(torch.equal(cnt_h, cnt_o)) and bool(torch.equal(views["ranges"][nz], st32.ranges[nz]))
    rep["instances_in_sample"] = int(cnt_o[tiles].sum())
    rep["n_contrib_mismatch_frac"] = (views["n_contrib"][mask] != st32.n_contrib[mask]).float().mean().item()
    m3 = mask[None].expand(3, H, W)
    img_err = ((outs[0] - st32.image).abs() / (1.0 + st32.image.abs()))[m3]
    rep["image_max_err_fp32"] = rep["image_max_err"] = img_err.max().item()
    rep["image_bad_frac"] = (img_err > 1e-5).float().mean().item()
    rep["image_bad_pixels"] = int((img_err.view(3, -1) > 1e-5).any(0).sum())
    d_err = ((outs[2] - st32.depth_img).abs() / (1.0 + st32.depth_img.abs()))[mask[None]]
    w_err = (outs[3] - st32.weights).abs()[mask[None]]
    rep["depth_max_err"], rep["weights_max_err"] = d_err.max().item(), w_err.max().item()
    rep["depth_bad_frac"] = (d_err > 1e-4).float().mean().item()
    rep["weights_bad_frac"] = (w_err > 1e-4).float().mean().item()
    rep["depth_bad_pixels"], rep["weights_bad_pixels"] = int((d_err > 1e-4).sum()), int((w_err > 1e-4).sum())
    rep["mean2D_max_err"] = (outs[4] - st32.mean2D).abs().max().item()
    rep["grad_rel_fp32"] = {k: rel_err(grads[k], gr32[k]) for k in GRAD_NAMES if grads.get(k) is not None and k in gr32}
    gr64 = None
    if check_fp64:
        st64, gr64 = O.render_and_grad(inp, s, g, dtype=torch.float64, discrete=O.discrete_of(st32), tiles=tiles)
        rep["grad_rel_fp64"] = {k: rel_err(grads[k], gr64[k]) for k in GRAD_NAMES if grads.get(k) is not None and k in gr64}
        rep["oracle32_vs_64"] = {k: rel_err(gr32[k], gr64[k]) for k in GRAD_NAMES if k in gr32 and k in gr64}
    if return_grads:
        return rep, dict(hip=grads, oracle32=gr32, oracle64=gr64)
    return rep


def tile_sort_paths(keys_sorted, ranges):
    """Which way through csrc/tile_sort.h every tile's list went on the tile-binned path, re-derived on the host from the sorted
    (tile << 32 | depth bits) keys and the ranges -- the same fp32 arithmetic as the kernels' bucket / slab functions:
      'wave256' / 'wave512'  one wave, bucket sort (half-size instance up to 256 entries)
      'block'                513..2048 entries: the whole workgroup, bucket sort
      'slabs'                2049..65536 entries: depth slabs through global memory, a wave per slab
      'network'              more than 65536 entries, or a slab that outgrows a wave (> 512 entries): bitonic network in global memory
      '+bitonic'             appended when more than 24 entries share a bucket: the LDS bitonic fallback of that size class
    Returns {path: number of lists}."""
    import numpy as np
    keys = keys_sorted.numpy().astype(np.uint64) & np.uint64(0xFFFFFFFF)
    out = {}
    for lo, hi in ranges.numpy().astype(np.int64):
        n = int(hi - lo)
        if n <= 1:
            continue
        k = keys[lo:hi].astype(np.int64)
        kmin, kmax = int(k[0]), int(k[-1])

        def crowded(kk, nb):
            scale = np.float32(nb) / (np.float32(int(kk[-1]) - int(kk[0])) + np.float32(1.0))
            bk = np.minimum(nb - 1, ((kk - kk[0]).astype(np.float32) * scale).astype(np.int64))
            return int(np.bincount(bk, minlength=nb).max()) > 24
        if n <= 512:
            path = ("wave256" if n <= 256 else "wave512") + ("+bitonic" if crowded(k, n) else "")
        elif n <= 2048:
            path = "block" + ("+bitonic" if crowded(k, n) else "")
        elif n <= 65536:
            K = min(256, (n + 255) // 256)
            scale = np.float32(K) / (np.float32(kmax - kmin) + np.float32(1.0))
            slab = np.minimum(K - 1, ((k - kmin).astype(np.float32) * scale).astype(np.int64))
            cnt = np.bincount(slab, minlength=K)
            if int(cnt.max()) > 512:
                path = "network"
            else:
                edges = np.concatenate([[0], np.cumsum(cnt)])
                bit = any(cnt[j] > 1 and crowded(k[edges[j]:edges[j + 1]], int(cnt[j])) for j in range(K))
                path = "slabs" + ("+bitonic" if bit else "")
        else:
            path = "network"
        out[path] = out.get(path, 0) + 1
    return out


def chunk_quadrant_counts(point_list, ranges, n_contrib, xy, conic, opacity, gx, CH, record_lists=None):
    """The backward's chunks (csrc/blend.hip, blend_bwd_scan_kernel), re-derived on the host: every tile's list is consumed back to
    front from its deepest contributor (the largest n_contrib of its pixels) in chunks of CH staged splats, and a wave's copy of the
    sums holds a slot for every staged splat whose 4x4-block reach mask (analysis_geometries.sub_masks: block_mask16's rule) touches
    the wave's quadrant.  Returns {tile: [(staged, largest per-quadrant reach count), ...]}, deepest chunk first; a chunk whose count
    exceeds the kernel's SL runs its group phase in two halves.
    record_lists = (point_list, ranges) of the opacity rule: the stock rule on the tile-binned path (COMPACT) stages its chunks from
    the compacted list of the positions that hold a gradient record -- the (tile, Gaussian) pairs the opacity rule emits -- starting
    at the number of those in front of the deepest contributor.  xy / conic / opacity: the preprocessed (P, .) arrays (numpy, fp64)."""
    import numpy as np
    from analysis_geometries import sub_masks, quadrant_groups
    pl = np.asarray(point_list).astype(np.int64)
    rg = np.asarray(ranges).astype(np.int64)
    nc = np.asarray(n_contrib)
    quads = quadrant_groups(4, 4)
    out = {}
    for t in range(rg.shape[0]):
        ty, tx = divmod(t, gx)
        tile_nc = nc[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]
        hi = int(tile_nc.max()) if tile_nc.size else 0               # the tile's deepest contributor: where its chunks start
        ids = pl[rg[t, 0]:rg[t, 0] + hi]
        if record_lists is not None:
            rpl, rrg = np.asarray(record_lists[0]).astype(np.int64), np.asarray(record_lists[1]).astype(np.int64)
            ids = ids[np.isin(ids, rpl[rrg[t, 0]:rrg[t, 1]])]
            hi = ids.size
        chunks = []
        while hi > 0:
            cnt = min(hi, CH)
            c = ids[hi - cnt:hi]
            m = sub_masks(xy[c, 0], xy[c, 1], conic[c, 0], conic[c, 1], conic[c, 2], opacity[c], np.full(cnt, tx * 16.0),
                          np.full(cnt, ty * 16.0), 4, 4)
            chunks.append((cnt, max(int(m[:, q].any(1).sum()) for q in quads)))
            hi -= cnt
        out[t] = chunks
    return out


INT_KEYS = ("radii_equal", "tiles_touched_equal", "rect_equal", "depth_bits_equal", "point_list_equal", "keys_equal",
            "ranges_equal")


def assert_ill_conditioned(rep, slack=3.0, floor=1e-4):
    """Cases whose fp32 evaluation is itself ill-conditioned (needle-shaped splats: the conic quadratic form and
    det(cov2D) cancel by ~1e5).  Integers stay bit-exact; floats are held to the accuracy the fp32 ORACLE achieves
    against the fp64 oracle on the same input: HIP may be at most `slack` x as far from fp64 as the fp32 oracle is."""
    for k in INT_KEYS:
        assert rep[k], f"{k} failed: {rep}"
    assert rep["num_rendered"][0] == rep["num_rendered"][1]
    assert rep["n_contrib_mismatch_frac"] <= 1e-3, rep["n_contrib_mismatch_frac"]
    # at most 2e-4 of the pixels may sit on a flipped threshold pair (same allowance as assert_report), none beyond 5e-3
    assert rep["image_outlier_frac_fp64"] <= 2e-4 and \
        rep["image_max_err_fp64"] <= max(5e-3, slack * rep["oracle32_vs_64_image_max"] + 1e-5), \
        (rep["image_outlier_frac_fp64"], rep["image_max_err_fp64"], rep["oracle32_vs_64_image_max"])
    for k, ref in rep["oracle32_vs_64"].items():
        if k in rep["grad_rel_fp64"]:
            assert rep["grad_rel_fp64"][k] <= slack * ref + floor, f"grad[{k}]: {rep['grad_rel_fp64'][k]:.3e} vs oracle32 {ref:.3e}"


def assert_image_bars(rep, threshold_pixels=0, mean2D_tol=1e-3):
    """The float OUTPUTS of a report (compare / compare_sampled): image |d| <= 1e-5 (1 + |x|), depth and weights <= 1e-4, on EVERY
    compared pixel.  threshold_pixels: how many pixels may sit on a flipped threshold pair instead -- alpha within an ulp of 1/255 or
    T (1 - alpha) of 1e-4, decided differently by the oracle's libm exp and the device's v_exp_f32; such a pixel changes by up to one
    splat's contribution (bounded at 5e-3 / 5e-2 / 2e-2 below).  0 by default; a test passes a number only for pixels it documents
    (round 5 accepted 2e-4 of the pixels on every case while every report but the full-size config 3 showed none)."""
    bad = (rep["image_bad_pixels"], rep["depth_bad_pixels"], rep["weights_bad_pixels"])
    assert max(bad) <= threshold_pixels, (bad, threshold_pixels, rep["image_max_err"])
    if threshold_pixels == 0:
        assert rep["image_max_err"] <= 1e-5 and rep["depth_max_err"] <= 1e-4 and rep["weights_max_err"] <= 1e-4
    else:
        assert rep["image_max_err"] <= 5e-3 and rep["depth_max_err"] <= 5e-2 and rep["weights_max_err"] <= 2e-2
    assert rep["mean2D_max_err"] <= mean2D_tol


def assert_report(rep, grad_tol=1e-4, skip_zero=(), tol_override=None, n_contrib_mismatch=0.0, threshold_pixels=0):
    """n_contrib_mismatch: fraction of pixels whose last contributor may differ from the oracle's.  0 by default -- n_contrib is an
    integer artefact; a test passes an allowance only where a documented threshold pair exists (T (1 - alpha) within an ulp of
    1e-4, or alpha of 1/255, decided differently by the oracle's libm exp and the device's v_exp_f32).  threshold_pixels: the same
    for the float outputs (assert_image_bars)."""
    for k in INT_KEYS:
        assert rep[k], f"{k} failed: {rep}"
    assert rep["num_rendered"][0] == rep["num_rendered"][1]
    assert rep["n_contrib_mismatch_frac"] <= n_contrib_mismatch, rep["n_contrib_mismatch_frac"]
    assert_image_bars(rep, threshold_pixels)
    # gradients: <= 1e-4 relative to the closer oracle (fp32 / fp64 walk), never worse than 2e-3 to the other one
    # (the two oracles themselves differ by that much when one of them flips a threshold pair: 'oracle32_vs_64')
    g32, g64 = rep.get("grad_rel_fp32", {}), rep.get("grad_rel_fp64", rep.get("grad_rel_fp32", {}))
    for k in g32:
        if k in skip_zero:
            continue
        best, worst = min(g32[k], g64.get(k, g32[k])), max(g32[k], g64.get(k, g32[k]))
        tb, tw = (tol_override or {}).get(k, (grad_tol, 2e-3))
        assert best <= tb, f"grad[{k}]: best-of {best:.3e} > {tb}: {rep}"
        assert worst <= tw, f"grad[{k}]: worst-of {worst:.3e} > {tw}: {rep}"
