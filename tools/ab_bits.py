#!/usr/bin/env python3
"""Bit-for-bit comparison of two BUILDS of the library: the product's libbags_raster.so against an alternative .so (the parent
commit's, built beforehand as tools/ab_lib.sh describes).  For a change that must not move a bit but whose generated code is not
instruction-identical to the parent's (csrc/projection.h: the projection chain shared by K1 and K9), so that results have to carry
what assembly identity cannot.

    tools/ab_bits.py <alternative .so> [--out DIR] [--timeout SECONDS]

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
the product only (before row_rebuild.h the call raised there): it must run, and is not compared."""
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
    return cases


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
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    cases = case_list()
    if not check_clamp(cases):
        print("FAIL: the narrow camera does not put visible Gaussians beyond the clamp on both axes")
        return 1
    if a.check_clamp:
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
        elif c.get("kind"):
            rows = ("row_rebuild", c["kind"])
            k9, tag = None, "%s %s" % rows
        if unstable:
            print(f"{c['name']:22s} NOT BIT-STABLE on the alternative itself, not counted ({tag}): " + " ".join(k.split("/")[1] for k in unstable))
            continue
        if rows:
            covered_rows.add(rows)
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
    miss_rows = sorted(map(str, want_rows - covered_rows))
    print(f"instances covered by stable cases: preprocess_bwd_kernel {len(covered_k9)} of 16, K1 {len(covered_k1)} of 4, "
          f"sh_grad_from_views {sum(r[0] == 'sh_grad_from_views' for r in covered_rows)} of 4, "
          f"colour backwards {sum(r[0] == 'sh_colors(_views)_bwd' for r in covered_rows)} of 7, "
          f"resized sets {sum(r[0] == 'row_rebuild' for r in covered_rows)} of 3")
    if miss9 or miss1 or miss_rows:
        print("FAIL: not covered:", miss9, miss1, miss_rows)
        return 1
    print("FAIL: %d tensors differ" % bad if bad else "OK: every tensor of every counted case is byte-equal")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
