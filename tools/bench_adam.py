"""The optimizer step of one training iteration, BASELINE config 3 shape (500 k Gaussians, SH degree 3 = 16 coefficients, six
parameter groups of 3 + 3 + 45 + 1 + 3 + 4 = 59 floats per Gaussian), gradients and radii from one real backward of the bench scene
at 1920x1080.  Time per step of
  a  torch.optim.Adam(l, lr=0.0, eps=1e-15) as the reference builds it (scene/gaussian_model.py:192-210)
  b  the same with fused=True
  c  GaussianAdam, dense (csrc/adam.hip, one launch)
  d  GaussianAdam, visible-only with the scene's own radii
  e  GaussianAdam, visible-only with a seeded 25 % mask
  f  GaussianAdam, dense, with the densification statistics folded in
  stats_ops  the four PyTorch ops of add_densification_stats + the max_radii2D line, alone
Each leg: warm-up, then --steps steps between two device events, median of --repeats.  Prints one JSON line.
Usage: python tools/bench_adam.py [--steps 200] [--repeats 5] [--only c]"""
import argparse, json, os, statistics, sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "bundle-adjusting-gaussian-splatting_amd")]
from bags_raster import GaussianAdam
from bags_raster.gaussians import GaussianBag
from bags_raster.loss import fused_photometric_loss
from bags_raster.render import render, PipelineParams
from bags_raster.synth import synth_scene, sphere_views

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LRS = (0.00016, 0.0025, 0.0025 / 20.0, 0.05, 0.005, 0.001)
COPY_RATE = 6.29e12            # bytes/s: what a float4 copy kernel reaches on the MI355X (8.0 TB/s HBM3E spec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200); ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20); ap.add_argument("--P", type=int, default=500_000)
    ap.add_argument("--only", default="", help="comma-separated legs (for kernel traces), e.g. c")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam needs the GPU: a time measured anywhere else says nothing")
    dev = torch.device("cuda", 0)
    P, W, H = args.P, 1920, 1080
    scene = synth_scene(P, 0, 0.5, 3)
    cam = sphere_views(1, W, H, noise=0.05, device=dev)[0]
    bag = GaussianBag.from_activated(scene, 3, device=dev)
    gt = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    out = render(cam, bag, PipelineParams(), torch.zeros(3, device=dev), 0.0, None, hybrid=False)
    fused_photometric_loss(out["render"], gt).backward()
    radii, view = out["radii"], out["viewspace_points"]
    leaves = [bag._xyz, bag._features_dc, bag._features_rest, bag._opacity, bag._scaling, bag._rotation]
    grads = [t.grad for t in leaves]
    floats = sum(t.numel() for t in leaves)
    mask25 = (torch.rand(P, generator=torch.Generator().manual_seed(7)) < 0.25).to(dev).to(torch.int32)

    def make(cls, **kw):
        params = [torch.nn.Parameter(t.detach().clone()) for t in leaves]
        for p, g in zip(params, grads):
            p.grad = g                                 # the same gradient tensors in every leg: only read
        return cls([{"params": [p], "lr": lr, "name": n} for p, lr, n in zip(params, LRS, NAMES)], lr=0.0, eps=1e-15, **kw)

    def stats_ops():
        vis = radii > 0
        bag.add_densification_stats(view, None, vis, False)
        bag.max_radii2D[vis] = torch.max(bag.max_radii2D[vis], radii[vis])

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                fn()
            e1.record(); torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / args.steps)
        return statistics.median(ms), min(ms), max(ms)
    legs = {
        "a_torch_adam": lambda: make(torch.optim.Adam).step,
        "b_torch_adam_fused": lambda: make(torch.optim.Adam, fused=True).step,
        "c_gaussian_adam_dense": lambda: make(GaussianAdam).step,
        "d_gaussian_adam_visible_radii": lambda: (lambda o: (lambda: o.step(visibility=radii)))(make(GaussianAdam)),
        "e_gaussian_adam_visible_25pct": lambda: (lambda o: (lambda: o.step(visibility=mask25)))(make(GaussianAdam)),
        "f_gaussian_adam_dense_stats": lambda: (lambda o: (lambda: o.step(stats=(bag, view, radii))))(make(GaussianAdam)),
        "stats_ops_pytorch": lambda: stats_ops,
    }
    only = [s for s in args.only.split(",") if s]
    res, spread = {}, {}
    for name, build in legs.items():
        if only and name.split("_")[0] not in only and name not in only:
            continue
        med, lo, hi = timed(build())
        res[name], spread[name] = med, [lo, hi]
        torch.cuda.empty_cache()
    line = {"metric": f"ms per optimizer step, {P} Gaussians x {floats // P} floats, median of {args.repeats} x {args.steps} steps",
            "device": torch.cuda.get_device_name(0), "P": P, "floats_per_gaussian": floats // P,
            "visible_fraction_radii": float((radii > 0).float().mean()), "ms": res, "min_max_ms": spread}
    if "c_gaussian_adam_dense" in res:
        moved = 7 * 4 * floats
        rate = moved / (res["c_gaussian_adam_dense"] * 1e-3)
        line.update(dense_bytes_moved=moved, dense_bytes_per_s=rate, dense_share_of_float4_copy_rate=rate / COPY_RATE)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
