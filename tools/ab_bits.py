#!/usr/bin/env python3
"""Bit-for-bit comparison of two BUILDS of the library: the product's libbags_raster.so against an alternative .so (the parent
commit's, built beforehand as tools/ab_lib.sh describes).  For a change that must not move a bit but whose generated code is not
instruction-identical to the parent's (csrc/projection.h: the projection chain shared by K1 and K9), so that results have to carry
what assembly identity cannot.

    tools/ab_bits.py <alternative .so> [--out DIR] [--timeout SECONDS]        (--check-rows: the CPU checks alone)

This process never touches the GPU.  It starts three fresh children one after the other, each under its own `timeout`: the
alternative (through BAGS_RASTER_LIB) twice, then the product, and stops at the first one that does not exit 0.  Every child runs
the same list of small cases and saves every output to an .npz: image, radii, depth, weights, mean2D, the integer artefacts of
debug_views, every gradient (pose gradients included).  Then bytes are compared: a case whose tensors differ between the two runs
of the ALTERNATIVE is not bit-stable on the parent build, is reported as such and does not count; every tensor of every other case
must be byte-equal between alternative and product.  One differing byte means an operation or its order changed.

The cases (160 x 120 image = 10 x 8 tiles, degree 3, tests/scenes.py:make_case with fixed seeds, P in {1, 257, 3000}: one lane, a
partial second workgroup, several blocks -- the kernels are one thread per Gaussian, the only edges are the workgroup's) are
crossed so that each of the 4 K1 kernels (SPLIT x with / without the tile count) and the 16 instances of preprocess_bwd_kernel
(COV3D x ACCUM x LIVE x EXTRA) runs in at least one stable case; one camera is narrow enough that visible Gaussians sit beyond the
1.3 x field-of-view clamp on each axis (checked on the CPU with the oracle before any child starts).  Exit status 0: every
counted tensor equal and every instance covered.

Since csrc/sh_rows.h (the SH gradient row write-out shared by K9, sh_grad_from_views_kernel and the sh_colors backwards) the list
also holds, at the same image size: steps of V = 3 views through rasterizer.FactoredSH, the second step accumulating (M = 16 packed
and split: sh_grad_from_views_kernel<0> / <1>; M = 9 packed and M = 4 split: the generic kernel; P in {129, 257, 3000}), and the
backwards of sh_colors and sh_colors_views with V = 3 and every gradient asked for (K in {16, 9, 4} packed and split, K = 1 packed,
P in {1, 257, 3000}: the store pass and the campos reduction both run).  They count as the others do.

Since csrc/row_rebuild.h (the rebuild of a resized set shared by densify_apply_kernel and mcmc_add_new_kernel) the list also holds
GaussianBag.densify_and_prune (P in {63, 1001}, N = 2 and, at 1001, N = 3; the children's normals given and from the in-kernel
generator; with and without optimizer state) and GaussianBag.add_new / relocate (P in {64, 65, 257, 4099}, SH degree 0 and 3, with
and without state, ``sampled`` given: the multinomial draw does not repeat at large P and must not decide a comparison).  Saved:
every parameter, both moments, the three statistics, provenance and the returned counts.  densify_and_prune at degree 0 runs on
the product only (before row_rebuild.h the call raised there): it must run, and is not compared.

Since csrc/ordered_sum.h (the ordered double sums and the quad access shared by the fused losses) the list also holds one ``kind``
per family -- depth_prior, normal_map, appearance, alpha, normal_prior, smooth, correspondence, warp, gaussian_reg, bilagrid and
bilagrid_tv -- each forward and backward with every gradient asked for; saved: the loss (or the output), the count, every gradient
and, where the wrapper keeps it for its backward, the stats rows.  Inputs are the tests' case modules' (tests/*_cases.py) at shapes
chosen for the sums: an image whose width is no multiple of 4 and whose last workgroup is partly filled, a shape whose finalize sees
fewer than 256 partial rows and one that sees more than 256 and no multiple of 256 (checked on the CPU, against the library's own
workspace size functions, before any child starts), the float4 and the element-by-element instance (the same case 4 bytes into its
allocations), every template instance of a family (L1 / Pearson, the four alpha modes, smooth's C x ORDER x NORM, gaussian_reg with
and without the filter, SUMS on and off in appearance and the reprojection backwards, both LMAX of the grid gradient), V = 1 and 3.
alpha's finalize and smooth's mean keep orders of their own (256 rows, 512 at most) and have no such row cases."""
import argparse
import itertools
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd"), os.path.join(ROOT, "tests")]

import numpy as np      # noqa: E402
import torch            # noqa: E402

W, H, DEG, SM = 160, 120, 3, 2.0
TILES = ((W + 15) // 16) * ((H + 15) // 16)
NARROW_FOVY = 0.15       # radians: the 1.3 x FoV bound lies 24 px (x) / 18 px (y) outside the image, the splats' 3 sigma reach ~100 px
SHIFT = (0.05, -0.02, 0.01)


def case_list():
    """One dict per case.  colour: packed (P,16,3) shs | split shs + shs_rest | precomp colours; cov: sr (scales + rotations) | cov3d."""
    cases = []

    def add(name, P, seed, colour="packed", cov="sr", accum=False, dense=-1, extra=False, binning="auto", tile_bounds="opacity",
            means2D=False, shift=False, cam="wide"):
        cases.append(dict(name=name, P=P, seed=seed, colour=colour, cov=cov, accum=accum, dense=dense, extra=extra, binning=binning,
                          tile_bounds=tile_bounds, means2D=means2D, shift=shift, cam=cam))
    # every instance of preprocess_bwd_kernel at P = 3000, the other switches rotating through the sixteen
    colours, bins, bounds = ("packed", "split", "precomp"), ("auto", "radix"), ("opacity", "aabb")
    for n, (cov, accum, dense, extra) in enumerate(itertools.product(("sr", "cov3d"), (False, True), (-1, 1), (False, True))):
        add(f"x{n:02d}", 3000, 20 + n, colours[n % 3], cov, accum, dense, extra, bins[(n // 3) % 2], bounds[(n // 2) % 2],
            means2D=(n % 4 == 1), shift=(n % 4 >= 2))
    # every K1 kernel (SPLIT x binning) at the workgroup's edges, both tile rules
    for P in (1, 257):
        for n, (colour, binning) in enumerate(itertools.product(("packed", "split"), ("auto", "radix"))):
            add(f"p{P}_{colour}_{binning}", P, 40 + n, colour, binning=binning, tile_bounds=bounds[n % 2], dense=(1 if n % 2 else -1),
                extra=(n >= 2), means2D=(n == 1), shift=(n != 1))
    add("p257_precomp_cov3d", 257, 50, "precomp", "cov3d", accum=True, dense=1, extra=True, shift=True)
    # the clamp branch: narrow camera, visible Gaussians beyond 1.3 x FoV on both axes
    add("narrow_packed", 3000, 60, "packed", cam="narrow")
    add("narrow_split_radix", 3000, 61, "split", binning="radix", tile_bounds="aabb", accum=True, dense=1, extra=True, cam="narrow")
    add("narrow_cov3d", 3000, 62, "precomp", "cov3d", dense=1, cam="narrow")
    # csrc/sh_rows.h: the factored SH gradient of a step of views, and the colour operators' backwards
    for P in (129, 257, 3000):
        for M, colour in ((16, "packed"), (16, "split"), (9, "packed"), (4, "split")):
            add(f"fsh_m{M}_{colour}_p{P}", P, 70 + M, colour)
            cases[-1].update(kind="factored", M=M)
    for P in (1, 257, 3000):
        for K, colour in ((16, "packed"), (16, "split"), (9, "packed"), (9, "split"), (4, "packed"), (4, "split"), (1, "packed")):
            add(f"shc_k{K}_{colour}_p{P}", P, 90 + K, colour)
            cases[-1].update(kind="shc", M=K)
    # csrc/row_rebuild.h: the resized set of densify_and_prune and add_new; relocate beside them (it shares the stage kernels)
    def resize(kind, name, P, seed, **kw):
        add(name, P, seed)
        cases[-1].update(kind=kind, **kw)
    for P, N in ((63, 2), (1001, 2), (1001, 3)):
        for given, state in itertools.product((True, False), repeat=2):
            resize("densify", f"dens_p{P}_n{N}_{'noise' if given else 'seed'}_{'state' if state else 'stateless'}", P, 110 + N, N=N, given=given, state=state)
    for kind, P, deg, state in itertools.product(("add_new", "relocate"), (64, 65, 257, 4099), (0, 3), (True, False)):
        resize(kind, f"{kind}_p{P}_deg{deg}_{'state' if state else 'stateless'}", P, 120 + deg, deg=deg, state=state)
    resize("densify", "dens_p65_deg0", 65, 1, N=2, given=True, state=True, deg=0, product_only=True)
    # csrc/ordered_sum.h: the fused losses.  `inst`: the template instance; `rows`: what the finalize must see (few / many / None)
    SHORT, WHOLE, TILED, PIXELS = (17, 67), (37, 260), (131, 515), (259, 257)      # W % 4 != 0 | W % 4 == 0 | 17 x 17 tiles | 261 chunks
    QUADS = (1030, 1028)                                                             # 1035 tiles of 256 quads: 259 rows

    def loss(kind, name, H=0, W=0, V=1, offset=False, rows=None, **kw):
        add(f"{kind}_{name}", 0, 0)
        cases[-1].update(kind=kind, H=H, W=W, V=V, offset=offset, rows=rows, **kw)
    for mode, space in (("pearson", "inverse"), ("l1", "depth")):
        loss("depth_prior", f"{mode}_short_v3", *SHORT, 3, rows="few", mode=mode, space=space, inst=(mode, False))
        loss("depth_prior", f"{mode}_vec_v3", *WHOLE, 3, mode=mode, space=space, inst=(mode, True))
        loss("depth_prior", f"{mode}_offset_v1", *WHOLE, 1, offset=True, mode=mode, space=space, inst=(mode, False))
    loss("depth_prior", "l1_many_v1", *QUADS, 1, rows="many", mode="l1", space="inverse", inst=("l1", True))
    for mode in ("cos", "l1"):
        loss("normal_map", f"{mode}_short_v3", *SHORT, 3, rows="few", mode=mode, inst=(mode, False))
        loss("normal_map", f"{mode}_vec_v3", *WHOLE, 3, mode=mode, inst=(mode, True))
        loss("normal_map", f"{mode}_offset_v1", *WHOLE, 1, offset=True, mode=mode, inst=(mode, False))
    loss("normal_map", "cos_many_v1", *QUADS, 1, rows="many", mode="cos", inst=("cos", True))
    for sums in (True, False):
        tag = "table" if sums else "images_only"
        loss("appearance", f"{tag}_short_v3", *SHORT, 3, rows="few" if sums else None, sums=sums, inst=(sums, False))
        loss("appearance", f"{tag}_vec_v3", *WHOLE, 3, sums=sums, inst=(sums, True))
        loss("appearance", f"{tag}_offset_v1", *WHOLE, 1, offset=True, sums=sums, inst=(sums, False))
    loss("appearance", "table_many_v1", *QUADS, 1, rows="many", sums=True, inst=(True, True))
    for mode in ("bce", "l1", "l2", "entropy"):                  # (515, 1028): a span of 518 quads, the second trip of a workgroup of 512
        for H, W, V, offset in ((5, 7, 3, False), (33, 70, 3, False), (33, 70, 1, True), (515, 1028, 1, False)):
            loss("alpha", f"{mode}_{H}x{W}_v{V}" + ("_offset" if offset else ""), H, W, V, offset=offset, mode=mode, inst=(mode, not offset))
    for mode in ("cos", "l1"):
        loss("normal_prior", f"{mode}_short_v3", *SHORT, 3, rows="few", mode=mode, inst=mode)
        loss("normal_prior", f"{mode}_many_v1", *TILED, 1, rows="many", mode=mode, inst=mode)
    for normals, order, normalize in ((False, 1, True), (False, 2, True), (False, 1, False), (False, 2, False), (True, 1, False), (True, 2, False)):
        tag = f"{'normal' if normals else 'depth'}_o{order}" + ("_norm" if normalize else "")
        loss("smooth", f"{tag}_short_v3", *SHORT, 3, rows="few", normals=normals, order=order, normalize=normalize, inst=(normals, order, normalize))
        loss("smooth", f"{tag}_many_v1", *TILED, 1, rows="many", normals=normals, order=order, normalize=normalize, inst=(normals, order, normalize))
    for sums in (True, False):
        tag = "views" if sums else "maps_only"
        loss("correspondence", f"{tag}_short_v3", *SHORT, 3, rows="few" if sums else None, sums=sums, delta=1.0, inst=sums)
        loss("correspondence", f"{tag}_many_v1", *PIXELS, 1, rows="many" if sums else None, sums=sums, delta=float("inf"), inst=sums)
        for C in (1, 3):
            loss("warp", f"c{C}_{tag}_short_v3", *SHORT, 3, rows="few" if sums else None, sums=sums, C=C, inst=(C, sums))
        loss("warp", f"c3_{tag}_many_v1", *PIXELS, 1, rows="many" if sums else None, sums=sums, C=3, inst=(3, sums))
    for filtered, selected in itertools.product((False, True), repeat=2):
        for P, rows in ((257, "few"), (3 * 1024 + 17, "few"), (256 * 1024 + 1000, "many")):
            if rows == "few" or selected == filtered:
                loss("gaussian_reg", f"p{P}_{'filter' if filtered else 'plain'}_{'select' if selected else 'all'}", P=P, rows=rows, filtered=filtered,
                     selected=selected, inst=filtered)
    for grid in ((16, 16, 8), (3, 2, 12)):                       # L <= 8 and L > 8: the two instances of the grid gradient
        loss("bilagrid", "g%dx%dx%d_v3" % grid, *SHORT, 3, grid=grid, inst=grid[2] > 8)
        loss("bilagrid", "g%dx%dx%d_v1" % grid, *SHORT, 1, grid=grid, inst=grid[2] > 8)
    loss("bilagrid_tv", "n23_5x4x3", grid=(5, 4, 3), N=23, rows="few", inst=None)
    loss("bilagrid_tv", "n4_16x16x8", grid=(16, 16, 8), N=4, rows="many", inst=None)
    return cases


# every template instance a family has, as its cases' `inst`: a stable case of each must have run
LOSS_INSTANCES = {
    "depth_prior": {(m, vec) for m in ("pearson", "l1") for vec in (False, True)},               # <VEC, L1>
    "normal_map": {(m, vec) for m in ("cos", "l1") for vec in (False, True)},                    # <VEC, L1>
    "appearance": {(sums, vec) for sums in (False, True) for vec in (False, True)},              # the backward's <VEC, SUMS>
    "alpha": {(m, vec) for m in ("bce", "l1", "l2", "entropy") for vec in (False, True)},        # <VEC, MODE>
    "normal_prior": {"cos", "l1"},                                                               # <L1>
    "smooth": {(False, 1, True), (False, 2, True), (False, 1, False), (False, 2, False), (True, 1, False), (True, 2, False)},   # (normals, ORDER, NORM)
    "correspondence": {False, True},                                                             # the backward's <SUMS>
    "warp": {(C, sums) for C in (1, 3) for sums in (False, True)},                               # <C, SUMS>
    "gaussian_reg": {False, True},                                                               # <FILTER>
    "bilagrid": {False, True},                                                                   # the grid gradient's LMAX: L > 8
    "bilagrid_tv": {None},
}
LOSS_KINDS = ("depth_prior", "normal_map", "appearance", "alpha", "normal_prior", "smooth", "correspondence", "warp", "gaussian_reg", "bilagrid",
              "bilagrid_tv")


def loss_rows(c):
    """(partial rows the finalize of case c adds, bytes of a row, the library's workspace size for one view) or None: from the constants
    of include/bags_raster.h as bags_raster._lib and the tests' case modules restate them."""
    import appearance_cases
    import depth_prior_cases
    import normal_prior_cases
    from bags_raster import _lib as L
    lib, k, H, W = L.load(), c["kind"], c["H"], c["W"]
    for fn in ("bags_depth_prior_workspace_size", "bags_normal_map_workspace_size", "bags_appearance_workspace_size", "bags_normal_prior_workspace_size",
               "bags_smooth_workspace_size", "bags_correspondence_workspace_size", "bags_warp_workspace_size", "bags_gaussian_reg_workspace_size",
               "bags_bilagrid_tv_workspace_size"):
        getattr(lib, fn).restype = __import__("ctypes").c_size_t
    if k == "depth_prior":
        return depth_prior_cases.slots(H, W), 8 * L.DEPTH_PRIOR_STATS, lib.bags_depth_prior_workspace_size(1, H, W)
    if k == "normal_map":
        return depth_prior_cases.slots(H, W), 8 * L.NORMAL_MAP_STATS, lib.bags_normal_map_workspace_size(1, H, W)
    if k == "appearance":
        return appearance_cases.slots(H, W), 8 * 16, lib.bags_appearance_workspace_size(1, H, W)
    if k == "normal_prior":
        return normal_prior_cases.tiles(H, W), 8 * L.NORMAL_PRIOR_STATS, lib.bags_normal_prior_workspace_size(1, H, W)
    if k == "smooth":                                            # (the mean rows behind the partial rows: 512 at most, an order of their own)
        mean = min(-(-H * W // 256), L.SMOOTH_MEAN_SLOTS)
        return -(-W // L.SMOOTH_TILE_W) * -(-H // L.SMOOTH_TILE_H), 8 * L.SMOOTH_PARTIALS, lib.bags_smooth_workspace_size(1, H, W) - -(-mean * 16 // 256) * 256
    if k in ("correspondence", "warp"):
        size = lib.bags_correspondence_workspace_size(1, H, W) if k == "correspondence" else lib.bags_warp_workspace_size(1, H, W)
        return -(-H * W // L.CORRESPONDENCE_CHUNK), 8 * L.CORRESPONDENCE_SUMS, size
    if k == "gaussian_reg":
        return -(-c["P"] // L.GAUSSIAN_REG_ROWS), 8 * L.GAUSSIAN_REG_STATS, lib.bags_gaussian_reg_workspace_size(c["P"])
    if k == "bilagrid_tv":
        Gx, Gy, Lz = c["grid"]
        return min(-(-c["N"] * 12 * Lz * Gy * Gx // L.BILAGRID_TV_BLOCK), L.BILAGRID_TV_MAX_BLOCKS), 8 * 4, lib.bags_bilagrid_tv_workspace_size(c["N"], Gx, Gy, Lz)
    return None


def check_rows(cases):
    """CPU: every case that is listed for its row count has it -- few: below 256, many: above 256 and no multiple of 256 (the second
    trip of ordered_rows_sum's loop and its remainder) -- and the count is what the library's size function hands out."""
    ok = True
    for c in cases:
        if c.get("kind") not in LOSS_KINDS or loss_rows(c) is None:
            continue
        rows, row_bytes, size = loss_rows(c)
        good = size == -(-rows * row_bytes // 256) * 256
        if c["rows"] == "few":
            good = good and 0 < rows < 256
        elif c["rows"] == "many":
            good = good and rows > 256 and rows % 256 != 0
        print(f"rows check {c['name']:44s} {rows:5d} rows of {row_bytes:3d} bytes, workspace {size:8d} bytes  wanted: {c['rows']}  {'ok' if good else 'FAIL'}")
        ok = ok and good
    return ok


def run_loss(c, dev):
    """GPU (child): one fused loss forward and backward, every gradient asked for; loss / output, count, stats and gradients are saved."""
    k, H, W, V = c["kind"], c["H"], c["W"], c["V"]

    def place(t, grad=False):                                    # at the start of an allocation, or -- offset -- 4 bytes into one
        if t is None:
            return None
        n = t.numel()
        buf = torch.empty(n + 4, dtype=t.dtype, device=dev)
        v = (buf[1:1 + n] if c["offset"] else buf[:n]).view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == (t.element_size() if c["offset"] else 0)
        return v.requires_grad_(True) if grad else v

    def each(ts, grad=False):
        return [place(t, grad) for t in ts]
    res, leaves, names, stats = {}, [], [], True
    if k == "depth_prior":
        import depth_prior_cases as M
        from bags_raster import depth_prior_loss
        m = M.make_case(H, W, V, c["mode"], c["space"])
        Ds, As = each(m["D"], True), each(m["A"], True)
        kw = {}
        if c["mode"] == "l1":
            table = m["table"].to(dev).requires_grad_(True)
            kw = dict(table=table, rows=m["rows"])
            leaves, names = [table], ["table"]
        out = depth_prior_loss(Ds, As, each(m["prior"]), each(m["mask"]), mode=c["mode"], space=c["space"], min_weight=M.MIN_WEIGHT, **kw)
        leaves, names, cot = Ds + As + leaves, [f"D{v}" for v in range(V)] + [f"A{v}" for v in range(V)] + names, m["cot"]
    elif k == "normal_map":
        import normal_map_cases as M
        from bags_raster import normal_map_loss
        m = M.case("generic", H, W, V)
        Ns = each(m["normal"], True)
        out = normal_map_loss(Ns, each(m["weights"]), each(m["target"]), each(m["mask"]), mode=c["mode"], min_weight=M.MIN_WEIGHT, min_norm=M.MIN_NORM)
        leaves, names, cot = Ns, [f"N{v}" for v in range(V)], M.cotangent(V)
    elif k == "alpha":
        import alpha_cases as M
        from bags_raster import alpha_loss
        m = M.case("generic", H, W, V)
        As = each(m["weights"], True)
        out = alpha_loss(As, None if c["mode"] == "entropy" else each(m["target"]), each(m["mask"]), mode=c["mode"], eps=m["eps"])
        leaves, names, cot = As, [f"A{v}" for v in range(V)], M.cotangent(V)
    elif k == "normal_prior":
        import normal_prior_cases as M
        from bags_raster import normal_prior_loss
        m = M.make_case(H, W, V, c["mode"])
        Ds, As = each(m["D"], True), each(m["A"], True)
        out = normal_prior_loss(Ds, As, each(m["prior"]), m["pinhole"], each(m["mask"]), mode=c["mode"], min_weight=M.MIN_WEIGHT, max_jump=M.MAX_JUMP)
        leaves, names, cot = Ds + As, [f"D{v}" for v in range(V)] + [f"A{v}" for v in range(V)], m["cot"]
    elif k == "smooth":
        import smooth_cases as M
        from bags_raster import depth_smooth_loss, normal_smooth_loss
        cfg = M.config(order=c["order"], normalize=c["normalize"], penalty="l1", eps=1e-2, guide="rgb", masked=True)
        Fs, As, Gs, ms, kw = M.arguments("generic", H, W, V, cfg, c["normals"], torch.float32, "cpu")
        Fs, As = each([t.detach() for t in Fs], True), each([t.detach() for t in As], not c["normals"])
        out = (normal_smooth_loss if c["normals"] else depth_smooth_loss)(Fs, As, each(Gs), each(ms), **kw)
        leaves = Fs + ([] if c["normals"] else As)
        names, cot = [f"F{v}" for v in range(V)] + ([] if c["normals"] else [f"A{v}" for v in range(V)]), M.cotangent(V)
    elif k in ("correspondence", "warp"):
        import correspondence_cases as CC
        import warp_cases as WC
        from bags_raster import correspondence_loss, warp_loss
        m = CC.make_case(H, W, V, c["delta"]) if k == "correspondence" else WC.make_case(H, W, V, c["C"], WC.EPSES[0])
        Ds, As, Vi, Vj = each(m["D"], True), each(m["A"], True), each(m["Vi"], c["sums"]), each(m["Vj"], c["sums"])
        if k == "correspondence":
            out = correspondence_loss(Ds, As, Vi, Vj, each(m["match"]), m["pin_i"], m["pin_j"], each(m["conf"]), delta=c["delta"],
                                      min_weight=CC.MIN_WEIGHT, min_depth=CC.MIN_DEPTH)
        else:
            dst = [[place(m[n][i]) if bool(m["has_dst"][i]) else None for i in range(V)] for n in ("D_dst", "A_dst")]
            out = warp_loss(Ds, As, Vi, Vj, each(m["color"]), each(m["image"]), m["pin_i"], m["pin_j"], each(m["conf"]), *dst, eps=m["eps"],
                            occlusion=WC.OCCLUSION, min_weight=WC.MIN_WEIGHT, min_depth=WC.MIN_DEPTH)
        leaves, names = Ds + As, [f"D{v}" for v in range(V)] + [f"A{v}" for v in range(V)]
        if c["sums"]:
            leaves, names = leaves + Vi + Vj, names + [f"Vi{v}" for v in range(V)] + [f"Vj{v}" for v in range(V)]
        cot = m["cot"]
    elif k == "gaussian_reg":
        import gaussian_reg_cases as M
        from bags_raster import REG_TERMS, gaussian_reg_loss
        m = M.make_case(c["P"], c["filtered"], c["selected"])
        x, r = place(m["opacity"], True), place(m["scaling"], True)
        out = gaussian_reg_loss(x, r, place(m["filter"]) if c["filtered"] else None, place(m["sel"]) if c["selected"] else None, REG_TERMS,
                                M.MAX_RATIO, M.MAX_SCALE)
        leaves, names, cot = [x, r], ["opacity", "scaling"], m["cot"]
    elif k == "appearance":
        import appearance_cases as M
        from bags_raster import apply_appearance
        m = M.make_case(H, W, V)
        table, xs = m["table"].to(dev).requires_grad_(c["sums"]), each(m["images"], True)
        outs = apply_appearance(xs, table, m["rows"], m["center"])
        leaves, names = xs + ([table] if c["sums"] else []), [f"image{v}" for v in range(V)] + (["table"] if c["sums"] else [])
        grads = torch.autograd.grad(outs, leaves, each(m["cot"]))
        res = {f"out{v}": o.detach() for v, o in enumerate(outs)}
        out = stats = None
    elif k == "bilagrid":
        import bilagrid_cases as M
        from bags_raster import apply_bilagrid
        m = M.make_case(c["grid"], H, W, V)
        grids, xs = m["grids"].to(dev).requires_grad_(True), [t.to(dev).requires_grad_(True) for t in m["images"]]
        outs = apply_bilagrid(xs, grids, m["rows"])
        leaves, names = xs + [grids], [f"image{v}" for v in range(V)] + ["grids"]
        grads = torch.autograd.grad(outs, leaves, [t.to(dev) for t in m["cot"]])
        res = {f"out{v}": o.detach() for v, o in enumerate(outs)}
        out = stats = None
    else:
        import bilagrid_cases as M
        from bags_raster import bilagrid_tv_loss
        grids = M.make_case(c["grid"], 3, 5, 1)["grids"][:c["N"]].to(dev).contiguous().requires_grad_(True)
        tv = bilagrid_tv_loss(grids)
        leaves, names = [grids], ["grids"]
        grads = torch.autograd.grad(tv, leaves, torch.tensor(1.25, device=dev))
        res = {"loss": tv.detach()}
        out = stats = None
    if out is not None:
        value, count = out
        res = {"loss": value.detach(), "count": count.detach()}
        if stats:                                                # the wrapper's first saved tensor: the stats rows its backward reads
            res["stats"] = value.grad_fn.saved_tensors[0].clone()
        grads = torch.autograd.grad(value, leaves, cot.to(dev, torch.float32))
    res.update({"grad_" + n: g for n, g in zip(names, grads)})
    res["num_rendered"] = torch.tensor([0])
    torch.cuda.synchronize(dev)
    return {n: t.cpu().numpy() for n, t in res.items()}


VIEWS = 3
LEAF = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}


def run_resize(c, dev):
    """GPU (child): one call of densify_and_prune / add_new / relocate on a seeded set; everything the call may write is saved."""
    import densify_reference as D
    import mcmc_reference as M
    from bags_raster import GaussianAdam
    from bags_raster.gaussians import GaussianBag
    P, kind, deg = c["P"], c["kind"], c.get("deg", 3)
    g = torch.Generator().manual_seed(3000 + c["seed"])
    if kind == "densify" and deg == 3:
        opt, stats, noise = D.make_case(P, c["seed"], GaussianAdam, dev, steps=3 if c["state"] else 0)
        if not c["state"]:
            opt.state.clear()
    else:
        opt, stats = M.make_case(P, c["seed"], GaussianAdam, dev, sh_degree=deg, state=c["state"])
        noise = torch.randn(P, 3, 3, generator=g)
    bag = GaussianBag(deg)
    for n, q in D.params(opt).items():
        setattr(bag, LEAF[n], q)
    bag.xyz_gradient_accum, bag.denom, bag.max_radii2D = stats["xyz_gradient_accum"], stats["denom"], stats["max_radii2D"]
    bag.active_sh_degree = deg
    res = {}
    if kind == "densify":
        how = dict(noise=noise[:, :c["N"]].contiguous().to(dev)) if c["given"] else dict(seed=1234 + P)
        out = bag.densify_and_prune(opt, N=c["N"], **how, **D.RULE)
        res["provenance"] = out.pop("provenance")
    elif kind == "add_new":
        A = int(1.05 * P) - P
        sampled = torch.randint(0, P, (A,), generator=g)
        sampled[-1] = sampled[0]                                     # a source drawn twice
        out = bag.add_new(opt, 10 * P, sampled=sampled.to(dev))
    else:
        dead = torch.zeros(P, dtype=torch.bool)
        dead[::3] = True
        alive = (~dead).nonzero().reshape(-1)
        sampled = alive[torch.randint(0, alive.numel(), (int(dead.sum()),), generator=g)]
        sampled[-1] = sampled[0]
        out = bag.relocate(opt, dead.to(dev), sampled=sampled.to(dev))
    res["counts"] = torch.tensor([int(v) for _, v in sorted(out.items())])
    for n, q in D.params(opt).items():
        assert q is getattr(bag, LEAF[n])
        res[n] = q.detach()
        if q in opt.state:
            res[n + ".exp_avg"], res[n + ".exp_avg_sq"] = opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]
    res.update(xyz_gradient_accum=bag.xyz_gradient_accum, denom=bag.denom, max_radii2D=bag.max_radii2D, num_rendered=torch.tensor([0]))
    torch.cuda.synchronize(dev)
    return {k: t.cpu().numpy() for k, t in res.items()}


def run_factored(c, dev):
    """GPU (child): two steps of VIEWS views with rasterizer.FactoredSH installed, the second accumulating on the first's gradients."""
    import math
    from bags_raster import GaussianRasterizationSettings, GaussianRasterizer
    from bags_raster import rasterizer as R
    from bags_raster.synth import sphere_views
    from scenes import camera_tensors
    x, _ = build_case(c)
    P, M = c["P"], c["M"]
    deg = {16: 3, 9: 2, 4: 1}[M]
    cams = sphere_views(VIEWS, W, H, noise=0.05)
    cots = [torch.randn(3, H, W, generator=torch.Generator().manual_seed(300 + v)).to(dev) for v in range(VIEWS)]
    leaf = lambda t: t.to(dev).clone().contiguous().requires_grad_(True)     # noqa: E731
    p = {k: leaf(x[k]) for k in ("means3D", "opacities", "scales", "rotations")}
    shs = x["shs"][:, :M]
    dc, rest = (leaf(shs[:, :1]), leaf(shs[:, 1:])) if c["colour"] == "split" else (leaf(shs), None)
    saved = (R.ACCUMULATE_IN_PLACE, R.FACTORED_SH, R.DENSE_PER_TILE)
    R.ACCUMULATE_IN_PLACE, R.DENSE_PER_TILE = True, -1
    try:
        for _ in range(2):
            fs = R.FactoredSH()
            R.FACTORED_SH = fs
            for cam, cot in zip(cams, cots):
                ct = camera_tensors(cam, dev)
                st = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
                                                   bg=torch.zeros(3, device=dev), scale_modifier=SM, viewmatrix=ct["viewmatrix"],
                                                   projmatrix=ct["projmatrix"], intrinsic=ct["intrinsic"], sh_degree=deg, campos=ct["campos"])
                img = GaussianRasterizer(st)(means3D=p["means3D"], means2D=torch.zeros(P, 3, device=dev, requires_grad=True), shs=dc, shs_rest=rest,
                                             opacities=p["opacities"], scales=p["scales"], rotations=p["rotations"])[0]
                img.backward(cot)
            R.FACTORED_SH = None
            fs.finish(p["means3D"], dc, rest)
    finally:
        R.ACCUMULATE_IN_PLACE, R.FACTORED_SH, R.DENSE_PER_TILE = saved
    res = {"grad_" + k: t.grad.detach() for k, t in p.items()}
    res["grad_shs"] = dc.grad.detach()
    if rest is not None:
        res["grad_shs_rest"] = rest.grad.detach()
    res["image"] = img.detach()
    res["num_rendered"] = torch.tensor([R.LAST_NUM_RENDERED])
    torch.cuda.synchronize(dev)
    return {k: t.cpu().numpy() for k, t in res.items()}


def run_shc(c, dev):
    """GPU (child): sh_colors (view 0) and sh_colors_views (VIEWS views) forward + backward, every gradient asked for."""
    from bags_raster import sh_colors, sh_colors_views
    x, _ = build_case(c)
    P, K = c["P"], c["M"]
    deg = {16: 3, 9: 2, 4: 1, 1: 0}[K]
    g = torch.Generator().manual_seed(2000 + c["seed"])
    centres = [torch.tensor([0.3 * v, -0.2, -4.0 + 0.5 * v]) + 0.1 * torch.randn(3, generator=g) for v in range(VIEWS)]
    cots = []
    for v in range(VIEWS):
        cot = torch.randn(P, 3, generator=g)
        cot[(2 + v)::5] = 0.0                            # rows without a cotangent, as for culled Gaussians
        cots.append(cot.to(dev))
    shs = x["shs"][:, :K]
    res = {}
    for tag in ("one", "views"):
        leaf = lambda t: t.to(dev).clone().contiguous().requires_grad_(True)     # noqa: E731
        xyz = leaf(x["means3D"])
        dc, rest = (leaf(shs[:, :1]), leaf(shs[:, 1:])) if c["colour"] == "split" else (leaf(shs), None)
        cps = [leaf(t) for t in centres]
        if tag == "one":
            outs = [sh_colors(deg, dc, xyz, cps[0], shs_rest=rest)]
        else:
            outs = list(sh_colors_views(deg, dc, xyz, cps, shs_rest=rest))
        torch.autograd.backward(outs, cots[:len(outs)])
        for v, o in enumerate(outs):
            res[f"{tag}_rgb{v}"] = o.detach()
            if cps[v].grad is not None:
                res[f"{tag}_grad_campos{v}"] = cps[v].grad.detach()
        res[f"{tag}_grad_shs"], res[f"{tag}_grad_xyz"] = dc.grad.detach(), xyz.grad.detach()
        if rest is not None:
            res[f"{tag}_grad_shs_rest"] = rest.grad.detach()
    res["num_rendered"] = torch.tensor([0])
    torch.cuda.synchronize(dev)
    return {k: t.cpu().numpy() for k, t in res.items()}


def build_case(c):
    from scenes import make_case
    scene, cam = make_case(c["P"], W, H, SM, DEG, seed=c["seed"], **({"fovy": NARROW_FOVY} if c["cam"] == "narrow" else {}))
    g = torch.Generator().manual_seed(1000 + c["seed"])
    P = c["P"]
    x = dict(scene)
    x["colors"] = torch.rand(P, 3, generator=g)
    L = torch.randn(P, 3, 3, generator=g) * (0.1 if c["cam"] == "wide" else 0.05)
    cov = L @ L.transpose(1, 2)
    x["cov6"] = torch.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], 1).contiguous()
    x["means2D"] = 0.01 * torch.randn(P, 3, generator=g) if c["means2D"] else torch.zeros(P, 3)
    x["g_img"] = torch.randn(3, H, W, generator=g)
    x["g_depth"] = torch.randn(1, H, W, generator=g)
    x["g_weights"] = torch.randn(1, H, W, generator=g)
    x["grad0"] = {k: 0.1 * torch.randn(*s, generator=g) for k, s in
                  (("means3D", (P, 3)), ("shs", (P, 16, 3)), ("colors", (P, 3)), ("opacities", (P, 1)), ("scales", (P, 3)),
                   ("rotations", (P, 4)), ("cov6", (P, 6)))}
    return x, cam


def check_clamp(cases):
    """CPU, oracle: the narrow camera's cases hold visible Gaussians beyond the clamp on each axis."""
    from oracle import raster_oracle as O
    from scenes import oracle_settings
    ok = True
    for c in cases:
        if c["cam"] != "narrow":
            continue
        x, cam = build_case(c)
        s = oracle_settings(cam, DEG, tile_bounds=c["tile_bounds"])
        pre = O.preprocess(x["means3D"], x["means2D"], torch.zeros(3), None if c["colour"] == "precomp" else x["shs"],
                           x["colors"] if c["colour"] == "precomp" else None, x["opacities"],
                           None if c["cov"] == "cov3d" else x["scales"], None if c["cov"] == "cov3d" else x["rotations"],
                           x["cov6"] if c["cov"] == "cov3d" else None, s)
        v = s.viewmatrix.reshape(16)
        m = x["means3D"]
        t = [m[:, 0] * v[j] + m[:, 1] * v[4 + j] + m[:, 2] * v[8 + j] + v[12 + j] for j in range(3)]     # no shift: tzs = tz
        vis = pre.radii > 0
        nx = int((vis & ((t[0] / t[2]).abs() > 1.3 * s.tanfovx)).sum())
        ny = int((vis & ((t[1] / t[2]).abs() > 1.3 * s.tanfovy)).sum())
        print(f"clamp check {c['name']}: visible {int(vis.sum())} of {c['P']}, clamped in x {nx}, in y {ny}")
        ok = ok and nx >= 3 and ny >= 3
    return ok


def run_case(c, dev):
    """GPU (child): one case through the op; returns {tensor name: numpy array}."""
    if c.get("kind") == "factored":
        return run_factored(c, dev)
    if c.get("kind") == "shc":
        return run_shc(c, dev)
    if c.get("kind") in ("densify", "add_new", "relocate"):
        return run_resize(c, dev)
    if c.get("kind") in LOSS_KINDS:
        return run_loss(c, dev)
    from bags_raster import GaussianRasterizer, debug_views
    from bags_raster import rasterizer as R
    from scenes import camera_tensors, hip_settings
    x, cam = build_case(c)
    R.ACCUMULATE_IN_PLACE = c["accum"]
    R.DENSE_PER_TILE = c["dense"]
    leaf = lambda t: t.to(dev).clone().contiguous().requires_grad_(True)     # noqa: E731
    ct = {k: v.clone().requires_grad_(True) for k, v in camera_tensors(cam, dev).items()}
    st = hip_settings(cam, DEG, dev, tensors=ct, tile_bounds=c["tile_bounds"], binning=c["binning"])
    st = st._replace(depth_weights_grad=c["extra"])
    p = dict(means3D=leaf(x["means3D"]), means2D=leaf(x["means2D"]), opacities=leaf(x["opacities"]),
             means2D_densify=torch.zeros(c["P"], 3, device=dev, requires_grad=True),
             shift_factors=leaf(torch.tensor(SHIFT if c["shift"] else (0.0, 0.0, 0.0))))
    g0 = x["grad0"]
    init = dict(means3D=g0["means3D"], opacities=g0["opacities"])
    if c["colour"] == "packed":
        p["shs"] = leaf(x["shs"]); init["shs"] = g0["shs"]
    elif c["colour"] == "split":
        p["shs"] = leaf(x["shs"][:, :1]); p["shs_rest"] = leaf(x["shs"][:, 1:])
        init["shs"] = g0["shs"][:, :1]; init["shs_rest"] = g0["shs"][:, 1:]
    else:
        p["colors_precomp"] = leaf(x["colors"]); init["colors_precomp"] = g0["colors"]
    if c["cov"] == "cov3d":
        p["cov3D_precomp"] = leaf(x["cov6"]); init["cov3D_precomp"] = g0["cov6"]
    else:
        p["scales"] = leaf(x["scales"]); p["rotations"] = leaf(x["rotations"])
        init["scales"] = g0["scales"]; init["rotations"] = g0["rotations"]
    if c["accum"]:                                   # the running sums the backward adds into
        for k, g in init.items():
            p[k].grad = g.to(dev).clone().contiguous()
    outs = GaussianRasterizer(st)(**p)
    heads, cots = [outs[0]], [x["g_img"].to(dev)]
    if c["extra"]:
        heads += [outs[2], outs[3]]; cots += [x["g_depth"].to(dev), x["g_weights"].to(dev)]
    torch.autograd.backward(heads, cots)
    res = {n: o.detach() for n, o in zip(("image", "radii", "depth", "weights", "mean2D"), outs)}
    for k, t in itertools.chain(p.items(), ct.items()):
        if t.grad is not None:
            res["grad_" + k] = t.grad.detach()
    res["num_rendered"] = torch.tensor([R.LAST_NUM_RENDERED])
    if c["colour"] != "split":                       # debug_views takes the packed layout
        with torch.no_grad():
            dv = debug_views(st, *[None if p.get(k) is None else p[k].detach() for k in
                                   ("means3D", "means2D", "shift_factors", "shs", "colors_precomp", "opacities", "scales", "rotations",
                                    "cov3D_precomp")])
        for k, t in dv.items():
            if torch.is_tensor(t):
                res["dbg_" + k] = t
        res["num_rendered"] = torch.tensor([dv["num_rendered"]])
    torch.cuda.synchronize(dev)
    return {k: t.cpu().numpy() for k, t in res.items()}


def child(path):
    assert torch.cuda.is_available(), "ab_bits.py: the children need the GPU"
    dev = torch.device("cuda:0")
    from bags_raster import _lib
    out = {}
    for c in case_list():
        if c.get("product_only") and os.environ.get("BAGS_RASTER_LIB"):
            continue
        for k, a in run_case(c, dev).items():
            out[f"{c['name']}/{k}"] = a
    np.savez(path, **out)
    print(f"child: {len(out)} tensors of {len(case_list())} cases from {_lib.LIB_PATH} -> {path}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("alternative", nargs="?")
    ap.add_argument("--out", help="where the children's .npz files go (default: a fresh temporary directory)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", metavar="NPZ", help=argparse.SUPPRESS)
    ap.add_argument("--check-clamp", action="store_true", help="only the CPU check of the narrow camera's cases")
    ap.add_argument("--check-rows", action="store_true", help="the CPU checks only, the loss cases' partial-row counts included")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    cases = case_list()
    if not check_clamp(cases):
        print("FAIL: the narrow camera does not put visible Gaussians beyond the clamp on both axes")
        return 1
    if a.check_clamp:
        return 0
    if not check_rows(cases):                            # (loads the library for its size functions: no GPU is touched)
        print("FAIL: a loss case does not have the partial rows it is listed for")
        return 1
    if a.check_rows:
        return 0
    if not a.alternative:
        ap.error("the alternative .so is required")
    alt = os.path.abspath(a.alternative)
    if not os.path.isfile(alt):
        ap.error(f"{alt}: no such file")
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    else:
        a.out = tempfile.mkdtemp(prefix="ab_bits_")
    runs = {}
    for tag, lib in (("alt_1", alt), ("alt_2", alt), ("product", None)):
        env = dict(os.environ)
        env.pop("BAGS_RASTER_LIB", None)
        if lib:
            env["BAGS_RASTER_LIB"] = lib
        path = os.path.join(a.out, tag + ".npz")
        rc = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", path], env=env).returncode
        if rc != 0:
            print(f"FAIL: child {tag} exited with {rc}; nothing further is started")
            return 1
        runs[tag] = np.load(path)
    same = lambda u, v: u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()     # noqa: E731
    bad, covered_k9, covered_k1, covered_rows = 0, set(), set(), set()
    for c in cases:
        if c.get("product_only"):
            n = sum(k.startswith(c["name"] + "/") for k in runs["product"].files)
            print(f"{c['name']:22s} product only: {n} tensors saved, not compared")
            bad += n == 0
            continue
        keys = sorted(k for k in runs["alt_1"].files if k.startswith(c["name"] + "/"))
        if sorted(k for k in runs["product"].files if k.startswith(c["name"] + "/")) != keys:
            print(f"{c['name']}: the product saved other tensors than the alternative"); bad += 1
            continue
        unstable = [k for k in keys if not same(runs["alt_1"][k], runs["alt_2"][k])]
        n_inst = int(runs["alt_1"][c["name"] + "/num_rendered"][0])
        k9 = (c["cov"] == "cov3d", c["accum"], c["dense"] > 0 and n_inst > c["dense"] * TILES, c["extra"])
        k1 = (c["colour"] == "split", c["binning"] == "auto")
        tag = "K9<COV3D,ACCUM,LIVE,EXTRA>=" + "".join("01"[b] for b in k9) + " K1<SPLIT>=%d%s" % (k1[0], ",count" if k1[1] else "")
        rows = None
        if c.get("kind") == "factored":                  # K9 runs too (ACCUM, no LIVE / EXTRA / COV3D): the raster cases cover it
            rows = ("sh_grad_from_views", c["M"] if c["M"] != 16 else (16, c["colour"]))
            k9, tag = None, "K9<..>=0100 + %s %s" % rows
        elif c.get("kind") == "shc":
            rows = ("sh_colors(_views)_bwd", c["M"], c["colour"])
            k9, tag = None, "%s K=%d %s" % rows
        elif c.get("kind") in LOSS_KINDS:
            rows = ("ordered_sum", c["kind"], c["inst"], c["rows"])
            k9, tag = None, "%s instance %s rows %s" % rows[1:]
        elif c.get("kind"):
            rows = ("row_rebuild", c["kind"])
            k9, tag = None, "%s %s" % rows
        if unstable:
            print(f"{c['name']:22s} NOT BIT-STABLE on the alternative itself, not counted ({tag}): " + " ".join(k.split("/")[1] for k in unstable))
            continue
        if rows:
            covered_rows.add(rows)
            if rows[0] == "ordered_sum":
                covered_rows.add(("ordered_sum rows", c["kind"], c["rows"]))
                covered_rows.add(("ordered_sum instance", c["kind"], c["inst"]))
        else:
            covered_k9.add(k9); covered_k1.add(k1)
        for k in keys:
            eq = same(runs["alt_1"][k], runs["product"][k])
            bad += not eq
            u = runs["alt_1"][k]
            print(f"{c['name']:22s} {k.split('/')[1]:24s} {str(u.dtype):8s} {str(u.shape):16s} {'equal' if eq else 'DIFFERS'}")
        print(f"{c['name']:22s} instances {n_inst}  {tag}")
    miss9 = [t for t in itertools.product((False, True), repeat=4) if t not in covered_k9]
    miss1 = [t for t in itertools.product((False, True), repeat=2) if t not in covered_k1]
    want_rows = {("sh_grad_from_views", (16, "packed")), ("sh_grad_from_views", (16, "split")), ("sh_grad_from_views", 9), ("sh_grad_from_views", 4)}
    want_rows |= {("sh_colors(_views)_bwd", K, col) for K in (16, 9, 4) for col in ("packed", "split")} | {("sh_colors(_views)_bwd", 1, "packed")}
    want_rows |= {("row_rebuild", kind) for kind in ("densify", "add_new", "relocate")}
    # csrc/ordered_sum.h: every instance of every family and both row counts, spelled out above, and every listed combination
    want_rows |= {("ordered_sum instance", k, inst) for k in LOSS_KINDS for inst in LOSS_INSTANCES[k]}
    want_rows |= {("ordered_sum", c["kind"], c["inst"], c["rows"]) for c in cases if c.get("kind") in LOSS_KINDS}
    want_rows |= {("ordered_sum rows", k, r) for k in LOSS_KINDS for r in ((None,) if k in ("alpha", "bilagrid") else ("few", "many"))}
    miss_rows = sorted(map(str, want_rows - covered_rows))
    print(f"instances covered by stable cases: preprocess_bwd_kernel {len(covered_k9)} of 16, K1 {len(covered_k1)} of 4, "
          f"sh_grad_from_views {sum(r[0] == 'sh_grad_from_views' for r in covered_rows)} of 4, "
          f"colour backwards {sum(r[0] == 'sh_colors(_views)_bwd' for r in covered_rows)} of 7, "
          f"resized sets {sum(r[0] == 'row_rebuild' for r in covered_rows)} of 3, "
          f"loss families {len({r[1] for r in covered_rows if r[0] == 'ordered_sum'})} of {len(LOSS_KINDS)} "
          f"in {sum(r[0] == 'ordered_sum' for r in covered_rows)} combinations of instance and row count")
    if miss9 or miss1 or miss_rows:
        print("FAIL: not covered:", miss9, miss1, miss_rows)
        return 1
    print("FAIL: %d tensors differ" % bad if bad else "OK: every tensor of every counted case is byte-equal")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
