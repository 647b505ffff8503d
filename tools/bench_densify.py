"""Densify-and-prune and the opacity reset at BASELINE config 3 shape (500 k Gaussians, 59 floats each, both Adam moments), state
and statistics from real iterations of the bench scene at 1920x1080 (GaussianAdam.step(stats=...)); thresholds from the scene's own
statistics (the medians, so that about half the rows are selected).  Time per call of
  a  the PyTorch route on the GPU: tests/densify_reference.py, the published clone / split / prune sequence with its optimizer surgery
  b  GaussianBag.densify_and_prune (csrc/densify.hip), and of its plan half alone (decide + scan + the host round trip)
  c  reset_opacity both ways
Every repeat starts from a fresh copy of the same state (made outside the timed region); median of --repeats, device events around
the call, which include the host work between the launches because that is part of what the call costs.  Prints one JSON line.
Usage: python tools/bench_densify.py [--repeats 5] [--iters 3] [--only b]"""
import argparse, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd"), os.path.join(ROOT, "tests")]
import densify_reference as D
from bags_raster import GaussianAdam, _lib as L
from bags_raster.gaussians import GaussianBag
from bags_raster.loss import fused_photometric_loss
from bags_raster.render import render, PipelineParams
from bags_raster.synth import synth_scene, sphere_views

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LEAF = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling", "rotation": "_rotation"}
LRS = (0.00016, 0.0025, 0.0025 / 20.0, 0.05, 0.005, 0.001)
COPY_RATE = 6.29e12            # bytes/s of a float4 copy kernel on the MI355X (profiles/adam/NOTES.md)
ROW_BYTES = 59 * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--P", type=int, default=500_000); ap.add_argument("--only", default="", help="comma-separated legs: a, b, c")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_densify needs the GPU: a time measured anywhere else says nothing")
    D.MARGINS = D.PROVENANCE = False        # the tests' bookkeeping (margins, provenance map) is no part of the route that is timed
    dev = torch.device("cuda", 0)
    P, W, H = args.P, 1920, 1080
    scene = synth_scene(P, 0, 0.5, 3)
    cam = sphere_views(1, W, H, noise=0.05, device=dev)[0]
    bag0 = GaussianBag.from_activated(scene, 3, device=dev)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    opt0 = GaussianAdam([{"params": [getattr(bag0, LEAF[n])], "lr": lr, "name": n} for n, lr in zip(NAMES, LRS)], lr=0.0, eps=1e-15)
    for _ in range(args.iters):
        for t in bag0.leaves():
            t.grad = None
        out = render(cam, bag0, PipelineParams(), torch.zeros(3, device=dev), 0.0, None, hybrid=False)
        fused_photometric_loss(out["render"], gt).backward()
        opt0.step(stats=(bag0, out["viewspace_points"], out["radii"]))
    stats0 = {k: getattr(bag0, k) for k in ("xyz_gradient_accum", "denom", "max_radii2D")}
    g = (stats0["xyz_gradient_accum"] / stats0["denom"]).nan_to_num(0.0)
    smax = torch.exp(bag0._scaling.detach()).max(dim=1).values
    rule = dict(max_grad=float(g[g > 0].median()), min_opacity=0.005, extent=float(smax.median()) / 0.01, max_screen_size=20, percent_dense=0.01)
    noise = torch.randn(P, 2, 3, generator=torch.Generator().manual_seed(3)).to(dev)

    def fresh(cls):
        opt = D.clone_optimizer(opt0, device=dev, opt_cls=cls)
        bag = GaussianBag(3)
        for n, q in D.params(opt).items():
            setattr(bag, LEAF[n], q)
        for k, v in stats0.items():
            setattr(bag, k, v.clone())
        return opt, bag

    def timed(setup, fn):
        ms, last = [], None
        for rep in range(args.repeats + 1):                         # the first one warms up (allocator, code objects)
            state = setup()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last = fn(*state)
            e1.record(); torch.cuda.synchronize()
            if rep:
                ms.append(e0.elapsed_time(e1))
            del state
            torch.cuda.empty_cache()
        return statistics.median(ms), [min(ms), max(ms)], last

    def plan_only(opt, bag):
        lib = L.load()
        r = L.BagsDensifyRule(P, 2, rule["max_grad"], rule["min_opacity"], rule["percent_dense"] * rule["extent"], 0.1 * rule["extent"],
                              rule["max_screen_size"], 1, 0, 0, 0, noise.data_ptr(), bag.xyz_gradient_accum.data_ptr(), bag.denom.data_ptr(),
                              bag.max_radii2D.data_ptr(), bag._scaling.data_ptr(), bag._opacity.data_ptr())
        n = lib.bags_densify_workspace_size(P)
        ws = torch.empty(n, dtype=torch.uint8, device=dev)
        counts = (L.C.c_int64 * L.DENSIFY_COUNTS)()
        L.check(lib.bags_densify_plan(r, ws.data_ptr(), n, counts, torch.cuda.current_stream().cuda_stream), "bags_densify_plan")
        return list(counts)
    only = [s for s in args.only.split(",") if s]
    res, spread, counts = {}, {}, {}
    if not only or "a" in only:
        res["a_pytorch_route"], spread["a_pytorch_route"], r = timed(lambda: fresh(torch.optim.Adam),
                                                                     lambda o, b: D.densify_and_prune(o, {k: getattr(b, k) for k in stats0}, noise=noise, **rule))
        counts["a"] = {k: r[k] for k in ("clones", "split", "pruned", "P_new")}
    if not only or "b" in only:
        res["b_fused"], spread["b_fused"], r = timed(lambda: fresh(GaussianAdam), lambda o, b: b.densify_and_prune(o, noise=noise, **rule))
        counts["b"] = {k: r[k] for k in ("kept", "clones", "split", "pruned", "P_new")}
        res["b_plan_only"], spread["b_plan_only"], _ = timed(lambda: fresh(GaussianAdam), plan_only)
    if not only or "c" in only:
        res["c_reset_pytorch"], spread["c_reset_pytorch"], _ = timed(lambda: fresh(torch.optim.Adam), lambda o, b: D.reset_opacity(o))
        res["c_reset_fused"], spread["c_reset_fused"], _ = timed(lambda: fresh(GaussianAdam), lambda o, b: b.reset_opacity(o))
    line = {"metric": f"ms per call, {P} Gaussians x 59 floats x (param, exp_avg, exp_avg_sq), median of {args.repeats}",
            "device": torch.cuda.get_device_name(0), "P": P, "rule": rule, "counts": counts, "ms": res, "min_max_ms": spread}
    if "b_fused" in res:
        rows_read = counts["b"]["kept"] * 3 + (counts["b"]["P_new"] - counts["b"]["kept"])          # kept rows: all three arrays; new rows: the parameter
        rows_written = counts["b"]["P_new"] * 3
        moved = (rows_read + rows_written) * ROW_BYTES
        apply_ms = res["b_fused"] - res["b_plan_only"]
        line.update(bytes_moved=moved, apply_ms_by_difference=apply_ms, apply_share_of_float4_copy_rate=moved / (apply_ms * 1e-3) / COPY_RATE)
        if "a_pytorch_route" in res:
            line["speedup_b_over_a"] = res["a_pytorch_route"] / res["b_fused"]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
